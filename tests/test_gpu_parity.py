"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against (a) the golden vectors made
from the reference and (b) the CPU oracle on seeded synthetic batches.  Tolerance: the north star's 1e-4
max-abs on predicted trajectories; intermediates are held to the same bound."""
import os

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4   # BASELINE.json north_star: "within 1e-4 max-abs on predicted trajectories"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", H.GOLDEN)
def test_forward_matches_reference_golden(name, dev):
    from trajsde_amd.runtime import NoiseSpec
    batch, meta, out, mid = H.load_fixture(name)
    model, cfg = H.build_model(meta)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    data = batch.to(dev)
    o = model(data, noise=NoiseSpec(seed=int(meta["noise_seed"])))
    plain = int(meta.get("uncertain", 1)) == 0                            # DEC:56, DEC:100-101: no scale head, loc [K, N, T, 2]
    assert o["loc"].shape[-1] == (2 if plain else 4) == out["loc"].shape[-1]
    assert plain == (not any(k.startswith("decoder.scale") for k in model.state_dict()))
    assert H.maxdiff(o["loc"].cpu(), out["loc"]) <= TOL
    assert H.maxdiff(o["pi"].cpu(), out["pi"]) <= TOL
    assert torch.equal(o["reg_mask"].cpu(), out["reg_mask"])
    assert H.maxdiff(o["diff_in"].cpu(), out["diff_in"]) <= TOL
    assert H.maxdiff(o["diff_out"].cpu(), out["diff_out"]) <= TOL
    assert H.maxdiff(data.y.cpu(), out["y_rot"]) <= 1e-5          # forward rotates y in place (MODEL:83-84)
    assert H.maxdiff(data["rotate_mat"].cpu(), out["rotate_mat"]) <= 1e-6
    im = model.encoder.last_intermediates
    assert H.maxdiff(im["aa_out"].cpu(), mid["aa_out"]) <= TOL
    assert H.maxdiff(im["latent_ys"].cpu(), mid["latent_ys"]) <= TOL
    if plain:              # the reference's losses chunk loc | scale out of four channels (losses/L2.py:12): training without the head is refused
        with pytest.raises(NotImplementedError):
            model.train().training_step(batch.to(dev), 0, noise=NoiseSpec(seed=1))


@pytest.mark.parametrize("name", H.GOLDEN)
def test_stages_in_isolation_match_golden(name, dev):
    """each stage fed with the reference's own inputs: errors cannot cancel or hide across stages"""
    from trajsde_amd import philox
    from trajsde_amd.runtime import NoiseSpec, rotate_inputs
    from trajsde_amd.schedule import decoder_schedule
    batch, meta, out, mid = H.load_fixture(name)
    model, cfg = H.build_model(meta)
    model = model.to(dev)
    seed, K, T = int(meta["noise_seed"]), int(meta["num_modes"]), int(meta["future_steps"])
    N = batch.num_nodes
    data = batch.to(dev)
    data["rotate_mat"], _ = rotate_inputs(data)
    local, di, do, li, lo = model.encoder(data=data, noise=NoiseSpec(seed=seed))
    assert H.maxdiff(local.cpu(), mid["local_embed"]) <= TOL
    assert float(li.abs().max()) == 0.0 and float((lo - 1).abs().max()) == 0.0
    g = model.aggregator(data=data, local_embed=mid["local_embed"].to(dev))
    assert H.maxdiff(g.cpu(), mid["global_embed"]) <= TOL
    # decoder: in-kernel Philox and injected normals (host twin of the same stream) must both match
    sched = decoder_schedule(T, float(meta["max_fut_t"]))
    z = torch.from_numpy(np.stack([philox.normals(seed, philox.STREAM_DECODER, k, np.arange(K * N), 64)
                                   for k in range(sched.n_euler)])).to(dev)
    for noise in (NoiseSpec(seed=seed), NoiseSpec(seed=0, z_dec=z)):
        dec = model.decoder(data=data, local_embed=mid["local_embed"].to(dev), global_embed=mid["global_embed"].to(dev), noise=noise)
        assert H.maxdiff(dec["loc"].cpu(), out["loc"]) <= TOL
        assert H.maxdiff(dec["pi"].cpu(), out["pi"]) <= TOL


@pytest.mark.parametrize("S,n,L,K,T,max_t,kw", [
    (4, 24, 12, 6, 20, 2.0, dict(mixed_source=True, history_dropout=0.4)),
    (3, 40, 20, 3, 30, 3.0, dict(source=1)),
    (2, 17, 5, 2, 5, 0.5, dict(nus_sparsity=True)),
    (1, 1, 3, 2, 5, 0.5, dict()),                 # a scene with a single actor: no edges at all
    (2, 11, 4, 20, 50, 5.0, dict(mixed_source=True)),   # the stress configuration's K=20 modes and 51 Euler steps
])
def test_forward_matches_oracle_on_synthetic(S, n, L, K, T, max_t, kw, dev):
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    batch = synth(S=S, n=n, L=L, F=T, box=120.0, seed=100 + n, **kw)
    model, cfg = H.build_model(K, T, max_t, init_seed=7)
    want = H.oracle_forward(model, cfg, batch, noise_seed=55)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    o = model(batch.to(dev), noise=NoiseSpec(seed=55))
    assert model.encoder.last_intermediates["E_aa"] == want["aa_edges"]          # identical edge sets (index work is exact)
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(o[key].cpu(), want[key]) <= TOL, key
    assert torch.equal(o["reg_mask"].cpu(), want["reg_mask"])


def test_degenerate_graphs(dev):
    """no agent-agent edges at all (every scene has a single actor), no lane-actor edges, duplicated edges"""
    from trajsde_amd.data import collate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 2, 5
    model, cfg = H.build_model(K, T, 0.5, init_seed=4)
    lonely = collate([synth(S=1, n=1, L=2, F=T, box=30.0, seed=60 + i) for i in range(3)])          # E = 0
    far = synth(S=2, n=5, L=3, F=T, box=40.0, seed=70)
    far["lane_actor_vectors"] = far["lane_actor_vectors"] + 1000.0                                    # every lane beyond the radius
    dup = synth(S=1, n=6, L=3, F=T, box=40.0, seed=71)
    dup["edge_index"] = torch.cat([dup["edge_index"], dup["edge_index"][:, :7]], dim=1)               # repeated edges count twice
    dup["edge_index"] = dup["edge_index"][:, torch.randperm(dup["edge_index"].shape[1], generator=torch.Generator().manual_seed(3))]
    gpu = None
    for batch in (lonely, far, dup):
        want = H.oracle_forward(model, cfg, batch, noise_seed=8)
        gpu = gpu or model.to(dev)
        o = gpu(batch.to(dev), noise=NoiseSpec(seed=8))
        for key in ("loc", "pi", "diff_in", "diff_out"):
            assert H.maxdiff(o[key].cpu(), want[key]) <= TOL, key


def test_edge_order_invariance(dev):
    """the CSR rows are put in canonical order, so permuting the input edge list changes nothing, bit for bit"""
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 2, 5
    model, cfg = H.build_model(K, T, 0.5, init_seed=4)
    model = model.to(dev)
    a = synth(S=3, n=12, L=5, F=T, box=60.0, seed=81, history_dropout=0.3)
    b = H.clone_batch(a)
    g = torch.Generator().manual_seed(5)
    b["edge_index"] = a["edge_index"][:, torch.randperm(a["edge_index"].shape[1], generator=g)]
    perm = torch.randperm(a["lane_actor_index"].shape[1], generator=g)
    b["lane_actor_index"], b["lane_actor_vectors"] = a["lane_actor_index"][:, perm], a["lane_actor_vectors"][perm]
    oa = model(a.to(dev), noise=NoiseSpec(seed=3))
    ob = model(b.to(dev), noise=NoiseSpec(seed=3))
    assert torch.equal(oa["loc"], ob["loc"]) and torch.equal(oa["pi"], ob["pi"])


def test_scene_independence_and_sharding_invariance(dev):
    """scenes never interact; with global row ids the Philox stream survives re-sharding"""
    from trajsde_amd.data import collate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 3, 5
    model, cfg = H.build_model(K, T, 0.5, init_seed=9)
    model = model.to(dev)
    a = synth(S=1, n=9, L=4, F=T, box=60.0, seed=31)
    b = synth(S=1, n=13, L=6, F=T, box=60.0, seed=32)
    both = collate([a, b])
    na, nb = a.num_nodes, b.num_nodes

    def ids(lo, hi):
        return torch.arange(lo, hi, dtype=torch.int32, device=dev)

    # global ids: actors 0..na+nb-1, fake agents na+nb.., decoder rows k*(na+nb)+actor
    tot = na + nb
    full = NoiseSpec(seed=77, fake_row_ids=ids(0, 2), enc_row_ids=torch.cat([ids(0, tot), ids(tot, tot + 2)]),
                     dec_row_ids=torch.cat([ids(k * tot, (k + 1) * tot) for k in range(K)]))
    o2 = model(both.to(dev), noise=full)
    part = NoiseSpec(seed=77, fake_row_ids=ids(1, 2), enc_row_ids=torch.cat([ids(na, tot), ids(tot + 1, tot + 2)]),
                     dec_row_ids=torch.cat([ids(k * tot + na, (k + 1) * tot) for k in range(K)]))
    o1 = model(b.to(dev), noise=part)
    assert H.maxdiff(o2["loc"][:, na:].cpu(), o1["loc"].cpu()) <= 1e-5
    assert H.maxdiff(o2["pi"][na:].cpu(), o1["pi"].cpu()) <= 1e-5


def test_forward_ood_matches_reference_golden(dev):
    """the OOD path (MODEL:89-98, ENC:204-370): 10 stochastic encoder passes -> per-actor std"""
    _forward_ood_golden("ood_k3_t5", dev)


def test_forward_ood_matches_reference_golden_under_irregular_masks(dev):
    """... on the reference's own output for synth.irregular_masks rows (tests/golden/irregular_ood)"""
    _forward_ood_golden("ood_irregular_k3_t5", dev)


def _forward_ood_golden(name, dev):
    from test_oracle_golden import _load_ood
    from trajsde_amd.runtime import NoiseSpec
    batch, meta, out = _load_ood(name)
    model, cfg = H.build_model(meta)
    model = model.to(dev)
    model.ood = True
    o = model(batch.to(dev), noise=NoiseSpec(seed=int(meta["noise_seed"])))
    assert "stds" in o and "diff_in" not in o
    assert H.maxdiff(o["stds"].cpu(), out["stds"]) <= TOL
    assert H.maxdiff(o["loc"].cpu(), out["loc"]) <= TOL
    assert H.maxdiff(o["pi"].cpu(), out["pi"]) <= TOL


def _scene_of(big, s, n, L):
    """scene `s` (n actors, L lanes) cut out of a collated synthetic batch, as a batch of its own"""
    from trajsde_amd.data import TemporalData
    lo, hi = s * n, (s + 1) * n
    ei = big["edge_index"]
    keep = (ei[1] >= lo) & (ei[1] < hi)
    lai = big["lane_actor_index"]
    lkeep = (lai[1] >= lo) & (lai[1] < hi)
    return TemporalData(x=big["x"][lo:hi], positions=big["positions"][lo:hi], padding_mask=big["padding_mask"][lo:hi],
                        bos_mask=big["bos_mask"][lo:hi], rotate_angles=big["rotate_angles"][lo:hi], y=big["y"][lo:hi],
                        edge_index=ei[:, keep] - lo, lane_positions=big["lane_positions"][s * L:(s + 1) * L],
                        lane_paddings=big["lane_paddings"][s * L:(s + 1) * L],
                        lane_actor_index=lai[:, lkeep] - torch.tensor([[s * L], [lo]]),
                        lane_actor_vectors=big["lane_actor_vectors"][lkeep], agent_index=big["agent_index"][s:s + 1] - lo,
                        av_index=big["av_index"][s:s + 1] - lo, batch=torch.zeros(n, dtype=torch.long),
                        source=big["source"][s:s + 1], num_nodes=n)


def _full_size_properties(dev, name, scenes, oracle_scenes=None, seed=4242):
    """A BASELINE shape at full size, at the initial weights: (1) outputs are finite, scales > min_scale, shapes as MODEL:74-102
    returns them; (2) scene independence: a scene taken out of the big batch and run alone (same global Philox row ids) gives the
    same trajectories (<= 1e-5); (3) that scene alone matches the CPU oracle (<= 1e-4).  The whole batch against the float64
    oracle on the GPU, at trained-like weights too: test_gpu_full_size_oracle.py.
    Returns (model on the device, cfg, big batch on the host, the big batch's outputs)."""
    import restate
    from trajsde_amd.shard import global_noise_spec
    from trajsde_amd.synth import CONFIGS, synth
    spec = CONFIGS[name]
    K, T = spec["num_modes"], spec["future_steps"]
    S, n, L = spec["synth"]["S"], spec["synth"]["n"], spec["synth"]["L"]
    model, cfg = H.build_model(K, T, spec["max_fut_t"], init_seed=0)
    big = synth(**spec["synth"])
    counts = [n] * S
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    gpu = model.to(dev)
    o_big = gpu(H.clone_batch(big).to(dev), noise=global_noise_spec(seed, range(S), counts, K, device=dev))
    assert torch.isfinite(o_big["loc"]).all() and torch.isfinite(o_big["pi"]).all()
    assert float(o_big["loc"][..., 2:].min()) > cfg["decoder"]["kwargs"]["min_scale"]
    assert tuple(o_big["loc"].shape) == (K, S * n, T, 4) and tuple(o_big["pi"].shape) == (S * n, K)
    # the same forward eight more times: the same bits (millions of tiles -- a timing-dependent low-order error shows up here, not on
    # fixtures)
    for _ in range(8):
        o_again = gpu(H.clone_batch(big).to(dev), noise=global_noise_spec(seed, range(S), counts, K, device=dev))
        assert torch.equal(o_again["loc"], o_big["loc"]) and torch.equal(o_again["pi"], o_big["pi"])
    for s in scenes:
        lo, hi = s * n, (s + 1) * n
        one = _scene_of(big, s, n, L)
        ns = global_noise_spec(seed, [s], counts, K, device=dev)
        o_one = gpu(H.clone_batch(one).to(dev), noise=ns)
        assert H.maxdiff(o_one["loc"].cpu(), o_big["loc"][:, lo:hi].cpu()) <= 1e-5, s
        assert H.maxdiff(o_one["pi"].cpu(), o_big["pi"][lo:hi].cpu()) <= 1e-5, s
        if oracle_scenes is not None and s not in oracle_scenes:
            continue
        want = restate.forward(P, cfg, H.clone_batch(one), restate.PhiloxNoise(
            seed, enc_row_ids=ns.enc_row_ids.cpu().numpy(), dec_row_ids=ns.dec_row_ids.cpu().numpy(),
            fake_row_ids=ns.fake_row_ids.cpu().numpy()))
        assert H.maxdiff(o_one["loc"].cpu(), want["loc"]) <= TOL, s
        assert H.maxdiff(o_one["pi"].cpu(), want["pi"]) <= TOL, s
    _lib_check_range()
    return gpu, cfg, big, o_big


def _lib_check_range():
    from trajsde_amd import _lib
    _lib.check_range()                                                     # no fp16x3 operand left the fp16 range on the way


def test_full_size_config2_properties(dev):
    """BASELINE configs[1] at full size (64 scenes x 128 agents, K=6, T=20)"""
    _full_size_properties(dev, "config2", scenes=(0, 37))


def test_full_size_config3_properties(dev):
    """BASELINE configs[2] at its full shape (synth.CONFIGS["config3"]: 32 Argoverse-sourced scenes x 48 agents, 150 lanes, K=6,
    T=30 -> 31 Euler steps with the solver's micro-step; the synthetic stand-in for the Argoverse val split, CFG:88-96): finite /
    scale checks, eight bit-identical repeats, two scenes re-run alone (<= 1e-5) and against the oracle (<= 1e-4)"""
    _full_size_properties(dev, "config3", scenes=(0, 17))


def test_full_size_metric256_properties(dev):
    """the workload `bench.py`'s `value` is quoted on (synth.CONFIGS["metric256"]: 32 scenes x 256 agents, K=6, 20 SDE steps,
    the shape BASELINE.json's metric names): finite / scale checks on the whole batch, two scenes re-run alone with the same
    global Philox row ids (<= 1e-5) and against the oracle (<= 1e-4) -- MODEL:74-102 on CFG:17,106"""
    _full_size_properties(dev, "metric256", scenes=(0, 21))


def test_stress_shape_config5_fp32_and_bf16_state(dev):
    """BASELINE configs[4] at its own shape on one GPU (8 scenes x 1024 agents, K=20, 50 SDE steps = 51 Euler steps; the 8-GPU
    form is 8 of these, no collective).  fp32 state: the properties above, one 1024-agent scene against the oracle at the
    north-star tolerance.  Then `set_state_storage("bf16")` ("bf16 hidden state"): same Philox streams, every intra-stage
    [rows][64] row rounded to bf16 -- finite, and within the measured accuracy class of that storage type (<= 5e-2 on the
    positions of ~4 m trajectories; DESIGN.md section 4 "bf16 state storage"), asserted here so that a regression of either
    path is seen."""
    from trajsde_amd import runtime
    from trajsde_amd.shard import global_noise_spec
    from trajsde_amd.synth import CONFIGS
    spec = CONFIGS["config5"]
    S, n, K = spec["synth"]["S"], spec["synth"]["n"], spec["num_modes"]
    gpu, cfg, big, o32 = _full_size_properties(dev, "config5", scenes=(5,))
    assert tuple(o32["loc"].shape) == (20, 8 * 1024, 50, 4)
    prev = runtime.set_state_storage("bf16")
    try:
        o16 = gpu(H.clone_batch(big).to(dev), noise=global_noise_spec(4242, range(S), [n] * S, K, device=dev))
        torch.cuda.synchronize()
    finally:
        runtime.set_state_storage(prev)
    assert torch.isfinite(o16["loc"]).all() and torch.isfinite(o16["pi"]).all()
    d_xy = H.maxdiff(o16["loc"][..., :2].cpu(), o32["loc"][..., :2].cpu())
    d_sc = H.maxdiff(o16["loc"][..., 2:].cpu(), o32["loc"][..., 2:].cpu())
    assert 0.0 < d_xy <= 5e-2, d_xy                                         # a different accuracy class, and really switched on
    assert d_sc <= 5e-2, d_sc
    # the storage switch is back: the fp32 path reproduces itself bit for bit
    again = gpu(H.clone_batch(big).to(dev), noise=global_noise_spec(4242, range(S), [n] * S, K, device=dev))
    assert torch.equal(again["loc"], o32["loc"])


def test_bench_spawned_rank_runs_the_rccl_path(tmp_path):
    """`bench.py` as the driver launches it for N > 1, exercised with one GPU: TRAJSDE_BENCH_SPAWN=1 makes the GPU-less parent
    start its rank as a child process (`spawn_ranks`), TRAJSDE_BENCH_FORCE_DIST=1 makes that rank initialise
    torch.distributed over RCCL (`init_process_group("nccl", device_id=...)`), run the ranks-seen all-reduce, the timing
    barriers and the max-over-ranks reduction.  Launched in a fresh interpreter (never exec'd from this process, which has
    initialised the GPU).  train.py:35,54 is the reference's counterpart (Lightning spawning the DDP ranks)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(TRAJSDE_BENCH_SPAWN="1", TRAJSDE_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--windows", "1",
                        "--no-cpu-baseline", "--no-secondary"], env=env, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["config"]["rccl_ranks_seen"] == 1
    assert line["steps"] == 2 and line["value"] > 0 and line["unit"] == "scenes/s"
    assert line["roofline"]["streams"] == 1 and 0.0 < line["roofline"]["frac"] < 1.0
    assert line["roofline_corun"]["launches"] >= 2
    # the training leg of the N > 1 bench: driver.train's step at the configs[3] shape with the design's one
    # collective -- the two-slice gradient all-reduce -- issued over RCCL (one-rank communicator here), with and without it
    ts = line["train_scaling"]
    assert "error" not in ts, ts
    assert ts["ranks"] == 1 and ts["overlap"] is True and ts["bytes"] > 4 * 500_000 and 0 < ts["early_slice_bytes"] < ts["bytes"]
    assert ts["ms_per_step"] > 0 and ts["ms_per_step_without_collective"] > 0
    assert abs(ts["allreduce_exposed_ms"] - (ts["ms_per_step"] - ts["ms_per_step_without_collective"])) < 1e-9
    assert line["config4_train"]["ms_per_step"] == ts["ms_per_step"] and line["config4_train"]["loss_L2"] > 0


def test_bench_times_k_steps_and_dumps_the_last_one(tmp_path, dev):
    """`bench.py --steps K --dump-outputs DIR`: one window of exactly K timed forwards, `ms_per_step` its time over K, and DIR
    holds what the last of them returned, one float32 .npy per output tensor -- the same forward run here (the headline
    workload, init_seed=0 weights, that step's Philox seed) gives the same arrays"""
    import json
    import subprocess
    import sys
    import bench
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import CONFIGS, synth
    steps, warmup, out_dir = 3, 2, tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--no-cpu-baseline", "--no-secondary", "--no-train-step", "--dump-outputs", str(out_dir)],
                       timeout=900, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and len(line["timing"]["windows_ms"]) == 1
    assert abs(line["ms_per_step"] - line["timing"]["windows_ms"][0] / steps) < 1e-9
    spec = CONFIGS[bench.WORKLOAD]
    model = PredictionModelSDENet(**bench.build_cfg(spec), init_seed=0).eval().to(dev)
    with torch.no_grad():
        want = model(synth(**spec["synth"]).to(dev), noise=NoiseSpec(seed=10_000 + warmup + steps - 1))
    torch.cuda.synchronize()
    want = {k: v.float().cpu() for k, v in want.items() if torch.is_tensor(v)}
    assert sorted(p.name for p in out_dir.iterdir()) == sorted(k + ".npy" for k in want)
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 << 20
    for k, v in want.items():
        got = np.load(out_dir / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(v.shape), k
        assert H.maxdiff(torch.from_numpy(got), v) <= 1e-5, k


def test_dense_scene_1024_agents(dev):
    """stress shape of BASELINE config 5 (one 1024-agent scene, in-degree up to 1023, K=20, 50 -> 51 Euler steps):
    the segment softmax / CSR paths at maximum fan-in, checked against the oracle."""
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T, max_t = 20, 50, 5.0
    batch = synth(S=1, n=1024, L=64, F=T, box=80.0, seed=77, history_dropout=0.2)     # 80 m box: everyone within the radius
    model, cfg = H.build_model(K, T, max_t, init_seed=11)
    want = H.oracle_forward(model, cfg, batch, noise_seed=5, want_intermediates=True)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    o = model(batch.to(dev), noise=NoiseSpec(seed=5))
    assert model.encoder.last_intermediates["E_aa"] == want["aa_edges"]
    assert H.maxdiff(o["loc"].cpu(), want["loc"]) <= TOL
    assert H.maxdiff(o["pi"].cpu(), want["pi"]) <= TOL


@pytest.mark.parametrize("name", H.GOLDEN)
def test_preserve_side_effects_leaves_the_reference_edge_snapshots_on_the_batch(name, dev):
    """ENC:107-110 leaves edge_index_t / edge_attr_t (extended edge list incl. the fake agents' in-edges, no radius filter) on
    the batch; with preserve_side_effects=True so does this build -- compared with what the reference's own forward left"""
    from trajsde_amd.runtime import NoiseSpec
    batch, meta, out, mid = H.load_fixture(name)
    model, cfg = H.build_model(meta)
    model = model.to(dev)
    data = batch.to(dev)
    model(data, noise=NoiseSpec(seed=int(meta["noise_seed"])))
    assert "edge_index_0" not in data                                   # opt-in: the default forward does not spend time on them
    data = batch.to(dev)
    model(data, noise=NoiseSpec(seed=int(meta["noise_seed"])), preserve_side_effects=True)
    for t in range(21):
        assert torch.equal(data[f"edge_index_{t}"].cpu(), mid[f"edge_index_{t}"]), t
        assert H.maxdiff(data[f"edge_attr_{t}"].cpu(), mid[f"edge_attr_{t}"]) == 0, t


def _sorted_cols(*rows):
    """columns of an index matrix in lexicographic order (multiset comparison of edge lists)"""
    m = torch.stack([r.to(torch.int64).cpu() for r in rows])
    key = torch.zeros(m.shape[1], dtype=torch.int64)
    for r in m:
        key = key * (int(m.max()) + 1 if m.numel() else 1) + r
    return m[:, torch.argsort(key, stable=True)]


@pytest.mark.parametrize("S,n,L,kw", [
    (3, 14, 6, dict(mixed_source=True, history_dropout=0.4)),
    (2, 33, 9, dict(nus_sparsity=True)),
    (1, 1, 2, dict()),
    (4, 20, 5, dict(history_dropout=0.7)),
    (1, 160, 8, dict(mixed_source=True)),                                # rows of 159 in-edges: three ballot blocks, > 64 survivors per segment
    (5, 70, 12, dict(history_dropout=0.3, nus_sparsity=True)),           # rows straddling ballot-block boundaries at every offset
    (3, 33, 6, dict(mixed_source=True, irregular=True)),                 # synth.irregular_masks: gaps, rows padded at step 20 or always
])
def test_compacted_edge_lists_equal_the_oracle_edge_sets_exactly(S, n, L, kw, dev):
    """index work is exact: the compacted agent-agent (t, src, dst), global (src, dst) and lane-actor (lane, actor) lists are
    the oracle's lists as multisets, the rows are in canonical order, and the segment pointers are the CSR of the targets"""
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    from trajsde_amd.synth import irregular_masks
    K, T = 2, 5
    kw = dict(kw)
    irregular = kw.pop("irregular", False)
    batch = synth(S=S, n=n, L=L, F=T, box=130.0, seed=300 + n, **kw)
    if irregular:
        batch = irregular_masks(batch, 300 + n, T)
    if n > 1:                                                            # duplicated and shuffled input edges too
        g = torch.Generator().manual_seed(n)
        ei = torch.cat([batch["edge_index"], batch["edge_index"][:, :5]], dim=1)
        batch["edge_index"] = ei[:, torch.randperm(ei.shape[1], generator=g)]
    model, cfg = H.build_model(K, T, 0.5, init_seed=2)
    want = H.oracle_forward(model, cfg, batch, noise_seed=9)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    model(batch.to(dev), noise=NoiseSpec(seed=9))
    im = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.encoder.last_intermediates.items()}
    N, A = batch.num_nodes, batch["agent_index"].numel()
    Nt = N + A
    # agent-agent: ours = (sender actor, snapshot node t*Nt+i); oracle = (t*Nt + sender, t*Nt + i)
    t_of = torch.div(im["aa_dst"], Nt, rounding_mode="floor")
    ours = _sorted_cols(t_of * Nt + im["aa_src"], im["aa_dst"])
    assert torch.equal(ours, _sorted_cols(*want["aa_edge_list"]))
    assert torch.equal(_sorted_cols(im["g_src"], im["g_dst"]), _sorted_cols(*want["g_edge_list"]))
    assert torch.equal(_sorted_cols(im["la_lane"], im["la_dst"]), _sorted_cols(*want["al_edge_list"]))
    for dst, src, segptr, rows in ((im["aa_dst"], im["aa_src"], im["aa_segptr"], 21 * Nt), (im["g_dst"], im["g_src"], im["g_segptr"], N),
                                   (im["la_dst"], im["la_lane"], im["la_segptr"], N)):
        assert segptr.numel() == rows + 1 and int(segptr[0]) == 0 and int(segptr[-1]) == dst.numel()
        counts = torch.bincount(dst.to(torch.int64), minlength=rows)
        assert torch.equal(segptr[1:] - segptr[:-1], counts.to(torch.int32))      # CSR of the targets
        assert bool((dst[1:] >= dst[:-1]).all())                                   # target-major
        same = dst[1:] == dst[:-1]
        assert bool((src[1:][same] >= src[:-1][same]).all())                       # senders ascending inside a row


def _random_graph_cases(count, seed):
    """seeded shapes for the sweep below: scene counts, scene sizes (down to one actor), lane counts, box sizes from "everyone sees
    everyone" to "nobody sees anybody", every generator option, shuffled / duplicated / pruned input edge lists"""
    import random
    rnd = random.Random(seed)
    cases = []
    for i in range(count):
        kw = {}
        if rnd.random() < 0.5:
            kw["mixed_source"] = True
        elif rnd.random() < 0.5:
            kw["source"] = rnd.choice([0, 1])
        if rnd.random() < 0.6:
            kw["history_dropout"] = rnd.choice([0.1, 0.4, 0.8])
        if rnd.random() < 0.4 and kw.get("source", 0) != 1:
            kw["nus_sparsity"] = True
        cases.append((rnd.choice([1, 2, 3, 5]), rnd.choice([1, 2, 3, 7, 16, 17, 40, 65, 90]), rnd.choice([1, 2, 5, 11]),
                      rnd.choice([20.0, 60.0, 150.0, 600.0]), rnd.choice(["as is", "shuffled", "duplicated", "pruned"]), 1000 + i, kw))
    return cases


@pytest.mark.gpu
def test_scene_cached_global_attention_leaves_large_scenes_to_the_gathering_kernel(dev, tmp_path):
    """the default global attention (gattn_h3.hip k_global_attn_sc, TRAJSDE_REL_SPLIT=2) parks a scene's k_node / v_node rows in LDS,
    which holds 256 actors; a batch that mixes a 20-actor scene with a 270-actor one must come out the same -- the large scene's
    targets are taken by the gathering kernel launched beside it -- as with the fp32-matrix kernel (=0) and the gathering kernel
    alone (=1)"""
    import os
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path[:0] = [%r, %r]\n"
        "import helpers as H\n"
        "from trajsde_amd.data import collate\n"
        "from trajsde_amd.runtime import NoiseSpec\n"
        "from trajsde_amd.synth import synth\n"
        "m, cfg = H.build_model(6, 20, 2.0, init_seed=2)\n"
        "b = collate([synth(S=1, n=20, L=8, F=20, box=90.0, seed=9), synth(S=1, n=270, L=8, F=20, box=200.0, seed=10),\n"
        "             synth(S=1, n=33, L=8, F=20, box=90.0, seed=11)])\n"
        "o = m.to('cuda')(b.to('cuda'), noise=NoiseSpec(seed=6))\n"
        "torch.save({k: v.cpu() for k, v in o.items()}, sys.argv[1])\n") % (H.ROOT, os.path.join(H.ROOT, "tests"))
    outs = {}
    for mode, env in (("default", {"TRAJSDE_REL_SPLIT": "0"}), ("scene_cache", {}), ("split", {"TRAJSDE_REL_SPLIT": "1"})):
        path = str(tmp_path / (mode + ".pt"))
        subprocess.run([sys.executable, "-c", script, path], check=True, env={**os.environ, **env}, timeout=600)
        outs[mode] = torch.load(path)
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(outs["default"][key], outs["scene_cache"][key]) <= 2e-5, key
        assert H.maxdiff(outs["default"][key], outs["split"][key]) <= 2e-5, key


@pytest.mark.gpu
def test_scene_cached_global_attention_stands_down_for_edges_that_join_two_scenes(dev, tmp_path):
    """the scene-cached kernel reads a target's senders out of ITS scene's rows in LDS: right for the reference's collated graphs (every
    global edge joins two actors of one scene), wrong for an edge list that joins two scenes -- which the reference would accept.  Such a
    batch is detected on the device (k_scene_ptr) and handed to the gathering kernel whole: same trajectories as the fp32-matrix kernel"""
    import os
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path[:0] = [%r, %r]\n"
        "import helpers as H\n"
        "from trajsde_amd.runtime import NoiseSpec\n"
        "from trajsde_amd.synth import synth\n"
        "m, cfg = H.build_model(6, 20, 2.0, init_seed=2)\n"
        "b = synth(S=3, n=24, L=8, F=20, box=90.0, seed=9, mixed_source=True)\n"
        "extra = torch.tensor([[1, 30, 5, 60], [30, 1, 60, 5]], dtype=b['edge_index'].dtype)      # actors of scenes 0 / 1 and 0 / 2\n"
        "b['edge_index'] = torch.cat([b['edge_index'], extra], dim=1).contiguous()\n"
        "o = m.to('cuda')(b.to('cuda'), noise=NoiseSpec(seed=6))\n"
        "torch.save({k: v.cpu() for k, v in o.items()}, sys.argv[1])\n") % (H.ROOT, os.path.join(H.ROOT, "tests"))
    outs = {}
    for mode, env in (("default", {}), ("fp32_matrix", {"TRAJSDE_REL_SPLIT": "0"}), ("gathering", {"TRAJSDE_REL_SPLIT": "1"})):
        path = str(tmp_path / (mode + ".pt"))
        subprocess.run([sys.executable, "-c", script, path], check=True, env={**os.environ, **env}, timeout=600)
        outs[mode] = torch.load(path)
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(outs["default"][key], outs["fp32_matrix"][key]) <= 2e-5, key
        assert torch.equal(outs["default"][key], outs["gathering"][key]), key      # the gathering kernel took every target


@pytest.mark.parametrize("S,n,L,box,edges,seed,kw", _random_graph_cases(24, 11))
def test_graph_stage_on_randomised_shapes_equals_the_oracle_lists(S, n, L, box, edges, seed, kw, dev):
    """the graph stage (rewritten in round 5: seven launches) over a seeded sweep of shapes: the three compacted lists equal the
    oracle's as multisets, rows canonical, segment pointers the CSR of the targets -- in the exact form (lengths read back) AND in the
    sync-free form the inference forward uses (lengths stay on the device): the two forwards give the same trajectories"""
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 2, 5
    batch = synth(S=S, n=n, L=L, F=T, box=box, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed)
    ei = batch["edge_index"]
    if ei.shape[1] > 0:
        if edges == "duplicated":
            ei = torch.cat([ei, ei[:, : max(1, ei.shape[1] // 7)]], dim=1)
        if edges == "pruned":
            ei = ei[:, torch.rand(ei.shape[1], generator=g) < 0.6]
        if edges != "as is":
            ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
        batch["edge_index"] = ei.contiguous()
    model, cfg = H.build_model(K, T, 0.5, init_seed=2)
    want = H.oracle_forward(model, cfg, batch, noise_seed=seed)
    model = model.to(dev)
    model.encoder.capture_intermediates = True                        # the exact form, lists exported
    o = model(batch.to(dev), noise=NoiseSpec(seed=seed))
    im = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.encoder.last_intermediates.items()}
    N, A = batch.num_nodes, batch["agent_index"].numel()
    Nt = N + A
    t_of = torch.div(im["aa_dst"], Nt, rounding_mode="floor")
    assert torch.equal(_sorted_cols(t_of * Nt + im["aa_src"], im["aa_dst"]), _sorted_cols(*want["aa_edge_list"]))
    assert torch.equal(_sorted_cols(im["g_src"], im["g_dst"]), _sorted_cols(*want["g_edge_list"]))
    assert torch.equal(_sorted_cols(im["la_lane"], im["la_dst"]), _sorted_cols(*want["al_edge_list"]))
    for dst, src, segptr, rows in ((im["aa_dst"], im["aa_src"], im["aa_segptr"], 21 * Nt), (im["g_dst"], im["g_src"], im["g_segptr"], N),
                                   (im["la_dst"], im["la_lane"], im["la_segptr"], N)):
        assert segptr.numel() == rows + 1 and int(segptr[0]) == 0 and int(segptr[-1]) == dst.numel()
        assert torch.equal(segptr[1:] - segptr[:-1], torch.bincount(dst.to(torch.int64), minlength=rows).to(torch.int32))
        assert bool((dst[1:] >= dst[:-1]).all())
        same = dst[1:] == dst[:-1]
        assert bool((src[1:][same] >= src[:-1][same]).all())
    assert H.maxdiff(o["loc"].cpu(), want["loc"]) <= TOL and H.maxdiff(o["pi"].cpu(), want["pi"]) <= TOL
    model.encoder.capture_intermediates = False                       # the inference forward: sync-free where the build supports it
    o2 = model(batch.to(dev), noise=NoiseSpec(seed=seed))
    assert torch.equal(o2["loc"], o["loc"]) and torch.equal(o2["pi"], o["pi"])


def test_csr_rows_longer_than_the_lds_sort_buffer(dev):
    """a target with more than 4096 in-edges (and an actor near more than 4096 lanes) takes the global-memory path of the
    canonical row sort; the row length is not a power of two"""
    from trajsde_amd.data import TemporalData
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T, n, L = 2, 5, 4200, 4300
    batch = synth(S=1, n=n, L=L, F=T, box=30.0, seed=91)             # everyone within the radius of everyone
    g = torch.Generator().manual_seed(17)
    star = torch.stack([torch.arange(1, n), torch.zeros(n - 1, dtype=torch.int64)])          # every actor -> actor 0
    ring = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    ei = torch.cat([star, ring], dim=1)
    batch["edge_index"] = ei[:, torch.randperm(ei.shape[1], generator=g)]
    la = torch.stack([torch.arange(L), torch.zeros(L, dtype=torch.int64)])                   # every lane -> actor 0
    la = la[:, torch.randperm(L, generator=g)]
    batch["lane_actor_index"] = la
    batch["lane_actor_vectors"] = batch["lane_positions"][la[0], -1] - batch["positions"][la[1], 20]
    model, cfg = H.build_model(K, T, 0.5, init_seed=2)
    want = H.oracle_forward(model, cfg, batch, noise_seed=4)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    o = model(batch.to(dev), noise=NoiseSpec(seed=4))
    im = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.encoder.last_intermediates.items()}
    Nt = n + 1
    t_of = torch.div(im["aa_dst"], Nt, rounding_mode="floor")
    assert torch.equal(_sorted_cols(t_of * Nt + im["aa_src"], im["aa_dst"]), _sorted_cols(*want["aa_edge_list"]))
    assert torch.equal(_sorted_cols(im["la_lane"], im["la_dst"]), _sorted_cols(*want["al_edge_list"]))
    for dst, src in ((im["aa_dst"], im["aa_src"]), (im["la_dst"], im["la_lane"])):
        same = dst[1:] == dst[:-1]
        assert bool((src[1:][same] >= src[:-1][same]).all())
    assert H.maxdiff(o["loc"].cpu(), want["loc"]) <= TOL


def test_driver_metrics_match_oracle(dev):
    """the test.py-like loop (YAML -> registry -> test_step -> metrics) against the oracle's trajectories"""
    from trajsde_amd import driver
    from trajsde_amd.metrics import ADE_T, FDE_T, MR_T
    from trajsde_amd.synth import CONFIGS, synth
    spec = CONFIGS["config1"]
    K, T = spec["num_modes"], spec["future_steps"]
    cfg = H.our_cfg(K, T, spec["max_fut_t"])
    for m in cfg["metric_args"]:
        m["end_idcs"] = [T - 1, T - 1]
    model = driver.build_model(cfg, None, dev, init_seed=0)
    batches = [synth(**dict(spec["synth"], seed=500 + i)) for i in range(3)]
    got = driver.evaluate(model, [b.to(dev) for b in batches], seed=40)
    cpu_model, _ = H.build_model(K, T, spec["max_fut_t"], init_seed=0)
    want = [ADE_T("nuScenes", [T - 1] * 2), FDE_T("nuScenes", [T - 1] * 2), MR_T("nuScenes", [T - 1] * 2)]
    for i, b in enumerate(batches):
        o = H.oracle_forward(cpu_model, cfg, b, noise_seed=40 + i, want_intermediates=False)
        idx = b["agent_index"]
        for m in want:
            m.update(o["loc"][:, idx, :, :2], o["y"][idx], o["reg_mask"][idx], b["source"])
    for name, m in zip(("ADE_T", "FDE_T", "MR_T"), want):
        assert abs(got[name] - float(m.compute())) <= 1e-4, name


def test_dataset_fed_batches_match_oracle(dev, tmp_path):
    """flat scene shards -> mixed-grid dataset -> loader -> forward, against the oracle on the same batch; the
    HBM-resident store must give the same batch as the host one"""
    import numpy as np
    from test_dataset import BASE, _groups
    from trajsde_amd import driver
    from trajsde_amd.dataset import SceneLoader, nuArgoDataset
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.scene_store import write_shard
    z = np.load(os.path.join(H.ROOT, "tests", "golden_data", "mixds.npz"))
    for sub, name, group in (("nu/val", "a", "raw/nus"), ("argo/train", "b", "raw/argo")):
        os.makedirs(tmp_path / sub)
        write_shard(str(tmp_path / sub / f"{name}.safetensors"), _groups(z, group))
    roots = (str(tmp_path / "nu"), str(tmp_path / "argo"))
    host = nuArgoDataset("val", None, None, *roots, spec_args=BASE)
    resident = nuArgoDataset("val", None, None, *roots, spec_args=BASE, device=str(dev))
    (hb,) = list(SceneLoader(host, batch_size=6, device=dev))
    (rb,) = list(SceneLoader(resident, batch_size=6, device=dev))
    for k in hb.keys:
        if torch.is_tensor(hb[k]):
            assert rb[k].device.type == "cuda" and torch.equal(hb[k], rb[k]), k
    K, T, max_t = 3, 60, 6.0
    model, cfg = H.build_model(K, T, max_t, init_seed=5)
    want = H.oracle_forward(model, cfg, hb.to("cpu"), noise_seed=77, want_intermediates=False)
    o = model.to(dev)(hb, noise=NoiseSpec(seed=77))
    for key in ("loc", "pi"):
        assert H.maxdiff(o[key].cpu(), want[key]) <= TOL, key
    assert torch.equal(o["reg_mask"].cpu(), want["reg_mask"])
    cfg["datamodule_specific"]["kwargs"].update(val_batch_size=4, test_dataset_args={**BASE})
    batches = list(driver.datamodule_batches(cfg, dev, 0, 1, *roots))
    assert [int(b["batch"].max()) + 1 for b in batches] == [4, 2]
    res = driver.evaluate(model, batches)
    assert all(np.isfinite(v) for v in res.values()), res


def test_alternative_kernel_paths_agree(dev, tmp_path):
    """the default kernels (fused edge attention on paired tiles, fused decoder heads, cooperative recurrence, fused global
    attention) against
    the alternative kernel structures selected by the TRAJSDE_* switches: the single-tile kernels on the plain images
    (TRAJSDE_*_FP32=1: exact fp32 MFMA in a bf16x6 build, the same split-precision products in the default fp16x3
    build), the two-launch recurrence and the unfused global attention.  The switches are read once per process, so
    each mode runs in its own interpreter"""
    import os
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path[:0] = [%r, %r]\n"
        "import helpers as H\n"
        "from trajsde_amd.runtime import NoiseSpec\n"
        "from trajsde_amd.synth import synth\n"
        "m, cfg = H.build_model(6, 20, 2.0, init_seed=2)\n"
        "o = m.to('cuda')(synth(S=3, n=20, L=8, F=20, box=90.0, seed=9, mixed_source=True).to('cuda'), noise=NoiseSpec(seed=6))\n"
        "torch.save({k: v.cpu() for k, v in o.items()}, sys.argv[1])\n") % (H.ROOT, os.path.join(H.ROOT, "tests"))
    outs = {}
    for mode, env in (("split", {}), ("fp32", {"TRAJSDE_EDGE_FP32": "1", "TRAJSDE_NODE_FP32": "1", "TRAJSDE_DECODE_FP32": "1",
                                               "TRAJSDE_RECUR_LEGACY": "1", "TRAJSDE_GLOBAL_UNFUSED": "1"}),
                      ("one_tile", {"TRAJSDE_EDGE_PAIR": "0"}),
                      ("two_kernel", {"TRAJSDE_ATTN_FUSED": "0"}),
                      ("gattn_vector", {"TRAJSDE_GATTN_F32MM": "0", "TRAJSDE_REL_SPLIT": "0"}),
                      ("gattn_f32", {"TRAJSDE_REL_SPLIT": "0"}),
                      ("rel_split", {"TRAJSDE_REL_SPLIT": "1"}),
                      ("rel_split_scene_cache", {"TRAJSDE_REL_SPLIT": "2"}),
                      ("fallbacks", {"TRAJSDE_RECUR_LEGACY": "1", "TRAJSDE_GLOBAL_UNFUSED": "1", "TRAJSDE_NODE_FP32": "0"})):
        path = str(tmp_path / (mode + ".pt"))
        subprocess.run([sys.executable, "-c", script, path], check=True, env={**os.environ, **env}, timeout=600)
        outs[mode] = torch.load(path)
    # ... and the library refuses a switch whose kernel form it no longer carries instead of silently running the default
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "refused.pt")], env={**os.environ, "TRAJSDE_EDGE_TILE": "32"},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "TRAJSDE_EDGE_TILE" in r.stderr
    for key in ("loc", "pi", "diff_in", "diff_out"):
        assert H.maxdiff(outs["split"][key], outs["fp32"][key]) <= 2e-5, key
        assert H.maxdiff(outs["split"][key], outs["fallbacks"][key]) <= 2e-5, key      # two-launch recurrence, unfused global attention, two-half FFN
        # the fused edge attention (default) against its two-kernel form (per-edge v / logits through HBM, chunked softmax):
        # same products, a different order of the softmax accumulation
        assert H.maxdiff(outs["split"][key], outs["two_kernel"][key]) <= 2e-5, key
        assert torch.equal(outs["two_kernel"][key], outs["one_tile"][key]), key        # two tiles per wave: the same bits
        # the fp32-matrix global attention (gattn_f32.hip) against the vector form it replaced (attn.hip k_global_attn)
        assert H.maxdiff(outs["gattn_f32"][key], outs["gattn_vector"][key]) <= 2e-5, key
        # the default global attention since the end of round 6 (gattn_h3.hip k_global_attn_sc: fp16x3 products on rel / node rows that
        # their writers store as split operand pieces, a scene's k_node / v_node rows resident in LDS) against the fp32-matrix kernel on
        # fp32 rows it replaced (gattn_f32.hip k_global_attn_mf) ...
        assert H.maxdiff(outs["split"][key], outs["gattn_f32"][key]) <= 2e-5, key
        # ... against the gathering form on the same rows (k_global_attn_h3: what scenes beyond the cache take)
        assert H.maxdiff(outs["split"][key], outs["rel_split"][key]) <= 2e-5, key
        # ... and the explicit switch is the default
        assert torch.equal(outs["split"][key], outs["rel_split_scene_cache"][key]), key


@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1.0, 30.0, 1e3, 1e4])
def test_sde_step_matches_float64_over_state_magnitudes(scale, dev):
    """one Euler-Maruyama step through the C-ABI (trajsde_sde_step, the split-precision drift/diffusion MLPs) against the
    oracle's drift/diffusion evaluated in float64, for hidden states of very different magnitude and a ragged row count:
    the fp16 pieces of the split must not lose small states (fp16 subnormals) nor large ones"""
    import ctypes as C
    import restate
    from trajsde_amd import _lib
    from trajsde_amd.schedule import decoder_schedule
    model, cfg = H.build_model(6, 20, 2.0, init_seed=4)
    for p_ in model.decoder.lsde_func.parameters():                   # not the initial weights: biases are zero there
        with torch.no_grad():
            p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())))
    model = model.to(dev)
    rows = 16 * 7 + 5
    g = torch.Generator().manual_seed(11)
    y = torch.randn(rows, 64, generator=g) * scale
    z = torch.randn(1, rows, 64, generator=g)
    tab = np.ascontiguousarray(decoder_schedule(20, 2.0).step_table())
    k = 3
    t0, dt, sq, sn, cs = (float(v) for v in tab[k, :5])
    yd, zd, out = y.to(dev), z.to(dev).contiguous(), torch.empty(rows, 64, device=dev)
    nz = _lib.Noise(C.c_uint64(0), zd.data_ptr(), None)
    e = tab[k].ctypes.data_as(C.POINTER(C.c_float))
    _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), yd.data_ptr(), out.data_ptr(), e, 0, C.byref(nz),
                                           torch.cuda.current_stream().cuda_stream), "trajsde_sde_step")
    torch.cuda.synchronize()
    P = {k_: v.detach().cpu().double() for k_, v in model.decoder.state_dict().items()}
    y64 = y.double()
    f = restate.drift(P, "lsde_func.f_func", y64, sn, cs)
    gs = restate.diffusion(P, "lsde_func.g_func", y64, sn, cs)
    want = y64 + f * dt + gs * (z[0].double() * sq)                    # SDEINT:483
    err = float((out.cpu().double() - want).abs().max())
    assert err <= 5e-6 * max(1.0, scale), (scale, err)
    _lib.check_range()                                                  # in range: the guard stays quiet


def test_bf16_state_storage(dev):
    """BASELINE configs[4] "bf16 hidden state": the [rows][64] activations that stay inside a stage (relative-pose rows,
    aa_out, the decoder's initial states, the state of trajsde_sde_step) stored as bf16.  Not a 1e-4 mode: bf16 keeps 8
    significant bits, and what it costs is REPORTED here -- the test pins the observed level (a few 1e-3 on trajectories of a
    few metres, against 5e-6 with fp32 storage) so that a regression in the storage path shows, and checks that fp32 mode is
    untouched by the switch."""
    import ctypes as C
    from trajsde_amd import _lib, runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule
    from trajsde_amd.synth import synth
    K, T, max_t = 6, 20, 2.0
    batch = synth(S=3, n=40, L=10, F=T, box=110.0, seed=123, mixed_source=True, history_dropout=0.3)
    model, cfg = H.build_model(K, T, max_t, init_seed=5)
    want = H.oracle_forward(model, cfg, batch, noise_seed=77)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    assert runtime.state_storage() == "fp32"
    a = model(batch.to(dev), noise=NoiseSpec(seed=77))
    assert runtime.set_state_storage("bf16") == "fp32"
    try:
        b = model(batch.to(dev), noise=NoiseSpec(seed=77))
        aa_bf16 = model.encoder.last_intermediates["aa_out"]
        err = {k: H.maxdiff(b[k].cpu(), want[k]) for k in ("loc", "pi", "diff_in")}
        print("bf16 state storage vs oracle:", err, "aa_out", H.maxdiff(aa_bf16.cpu(), want["aa_out"]))
        assert H.maxdiff(aa_bf16.cpu(), want["aa_out"]) <= 2e-2 * float(want["aa_out"].abs().max())       # one bf16 rounding of a row
        assert err["loc"] <= 5e-2 and err["pi"] <= 5e-2 and err["loc"] > 1e-5                             # really a different mode
        with pytest.raises(_lib.TrajsdeError, match="fp32"):                                              # inference only
            model.train().training_step(batch.to(dev), 0, noise=NoiseSpec(seed=1)).backward()
        model.eval()
        # the step kernel on a bf16 state: one Euler-Maruyama step equals the fp32 step on the same (bf16-representable) state
        rows = 100
        tab = np.ascontiguousarray(decoder_schedule(T, max_t).step_table())
        e = tab[2].ctypes.data_as(C.POINTER(C.c_float))
        nz = _lib.Noise(C.c_uint64(3), None, None)
        st = torch.cuda.current_stream().cuda_stream
        y16 = torch.randn(rows, 64, device=dev).to(torch.bfloat16)
        o16 = torch.empty_like(y16)
        _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), y16.data_ptr(), o16.data_ptr(), e, 2, C.byref(nz), st))
        runtime.set_state_storage("fp32")
        y32 = y16.float()
        o32 = torch.empty_like(y32)
        _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), y32.data_ptr(), o32.data_ptr(), e, 2, C.byref(nz), st))
        torch.cuda.synchronize()
        assert torch.equal(o16, o32.to(torch.bfloat16))                                                    # same arithmetic, rounded once at the store
    finally:
        runtime.set_state_storage("fp32")
    c = model(batch.to(dev), noise=NoiseSpec(seed=77))
    assert torch.equal(a["loc"], c["loc"]) and H.maxdiff(c["loc"].cpu(), want["loc"]) <= TOL


def test_fp16_range_guard_is_loud(dev):
    """magnitudes the fp16 pieces cannot hold (>= 65504) are refused with TRAJSDE_ERR_UNSUPPORTED instead of saturating
    silently: a hidden state of 7e4 through trajsde_sde_step, an embedding element of 1e5 through the SDE decoder, a weight of
    1e5; and the flag is sticky until it is read.  (Every other site and route -- an aggregate of 7e4 through the node block of
    the aggregator among them -- is in tests/test_gpu_range_guard.py.)"""
    import ctypes as C
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec, rotate_inputs
    from trajsde_amd.schedule import decoder_schedule
    from trajsde_amd.synth import synth
    _lib.check_range()                                                  # start clean
    model, cfg = H.build_model(2, 5, 0.5, init_seed=4)
    model = model.to(dev)
    rows = 40
    tab = np.ascontiguousarray(decoder_schedule(5, 0.5).step_table())
    e = tab[1].ctypes.data_as(C.POINTER(C.c_float))
    nz = _lib.Noise(C.c_uint64(3), None, None)
    st = torch.cuda.current_stream().cuda_stream
    for scale, ok in ((6.0e4, True), (7.0e4, False)):
        y = torch.full((rows, 64), scale, device=dev)
        y[:, ::2] *= -1
        out = torch.empty_like(y)
        _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), y.data_ptr(), out.data_ptr(), e, 0, C.byref(nz), st))
        if ok:
            _lib.check_range()
        else:
            with pytest.raises(_lib.TrajsdeError, match="decoder SDE state"):
                _lib.check_range()
            _lib.check_range()                                          # reading cleared it
    # whole forward on a sane batch: quiet
    batch = synth(S=2, n=6, L=3, F=5, box=50.0, seed=5).to(dev)
    model(batch, noise=NoiseSpec(seed=1))
    _lib.check_range()
    # the decoder fed with an embedding row of 1e5
    batch["rotate_mat"], _ = rotate_inputs(batch)
    N = batch.num_nodes
    local = torch.randn(N, 64, device=dev)
    glob = torch.randn(2, N, 64, device=dev)
    glob[1, 3, 7] = 1.0e5
    model.decoder(data=batch, local_embed=local, global_embed=glob, noise=NoiseSpec(seed=1))
    with pytest.raises(_lib.TrajsdeError, match="decoder embedding inputs"):
        _lib.check_range()
    # a weight without an fp16 image
    with torch.no_grad():
        model.decoder.p("lsde_func.f_func.net.2.weight")[5, 5] = 1.0e5
    model.decoder(data=batch, local_embed=local, global_embed=glob[:, :, :].clamp(-10, 10), noise=NoiseSpec(seed=1))
    with pytest.raises(_lib.TrajsdeError, match="weight"):
        _lib.check_range()


def test_errors_are_loud(dev):
    from trajsde_amd import _lib
    from trajsde_amd.synth import synth
    model, cfg = H.build_model(2, 5, 0.5, init_seed=1)
    batch = synth(S=1, n=4, L=2, F=5, box=50.0, seed=1)
    with pytest.raises(_lib.TrajsdeError):
        model.to(dev)(batch)                      # CPU batch: the hot path has no CPU implementation
    L = _lib.lib()
    assert L.trajsde_decoder_forward(0, 1, 1, None, None, None, None, 0, None, 0.0, None, None, 0, None, None, None) != 0
    assert b"null" in L.trajsde_last_error() or b"empty" in L.trajsde_last_error()


@pytest.mark.parametrize("S,n,L,kw", [
    (3, 14, 6, dict(mixed_source=True, history_dropout=0.4)),
    (1, 1, 2, dict()),                                                   # no agent-agent edge at all
    (6, 90, 40, dict(nus_sparsity=True)),                                # E_aa > 65536: streams of more than one edge
    (3, 13, 6, dict(mixed_source=True, irregular=True)),                 # synth.irregular_masks: empty global segments, rows without a bos
])
def test_sync_free_forward_is_bitwise_the_exact_forward(S, n, L, kw, dev):
    """trajsde_graph_prepare_async leaves the list lengths on the device and hands the kernels bounds; the kernels derive the
    same stream cut from the device-side count, so the outputs are bit-identical -- and the graph can still be made exact
    for an entry point that needs host-side lengths"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    from trajsde_amd.synth import irregular_masks
    K, T = 3, 6
    kw = dict(kw)
    irregular = kw.pop("irregular", False)
    batch = synth(S=S, n=n, L=L, F=T, box=60.0, seed=5, **kw)
    if irregular:
        batch = irregular_masks(batch, 5, T)
    model, cfg = H.build_model(K, T, 0.5, init_seed=3)
    model = model.to(dev).eval()
    assert runtime.sync_free()                                           # the default
    outs = {}
    for mode in (True, False):
        prev = runtime.set_sync_free(mode)
        try:
            data = batch.to(dev)
            with torch.no_grad():
                o = model(data, noise=NoiseSpec(seed=12))
            gc = data["_trajsde_graph"]
            assert bool(gc.graph.exact) == (not mode)
            outs[mode] = ({k: v.clone() for k, v in o.items() if torch.is_tensor(v)}, gc.true_counts(), gc)
        finally:
            runtime.set_sync_free(prev)
    assert outs[True][1] == outs[False][1]
    assert {"loc", "pi", "diff_in", "diff_out"} <= set(outs[True][0])
    for k in outs[True][0]:
        assert torch.equal(outs[True][0][k], outs[False][0][k]), k
    gc = outs[True][2]
    bound = gc.graph.E_aa
    gc.make_exact()
    assert gc.graph.exact and gc.graph.E_aa == outs[False][1]["E_aa"] <= bound
    lists = gc.edge_lists()
    assert lists["aa_dst"].numel() == gc.graph.E_aa
    model.check_range()


def test_training_after_a_sync_free_forward_of_the_same_batch(dev):
    """the training entry points need exact list lengths: they make a graph left by a sync-free forward exact themselves"""
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 2, 5
    batch = synth(S=2, n=12, L=5, F=T, box=40.0, seed=8)
    model, cfg = H.build_model(K, T, 0.5, init_seed=4)
    model = model.to(dev)
    data = batch.to(dev)
    y0 = data.y.clone()
    model.eval()
    with torch.no_grad():
        model(data, noise=NoiseSpec(seed=3))
    assert not data["_trajsde_graph"].graph.exact
    model.train()
    data.y = y0
    loss = model.training_step(data, 0, noise=NoiseSpec(seed=3))
    loss.backward()
    assert torch.isfinite(loss)
    assert data["_trajsde_graph"].graph.exact


def test_graph_replay_is_the_eager_forward(dev):
    """runtime.GraphedForward: the whole inference forward (graph stage included) captured once and replayed; the Philox key is
    read from device memory, so a replay with seed s is bit-for-bit the eager forward with NoiseSpec(seed=s), and an in-place
    edit of the batch is seen by the next replay"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    K, T = 3, 6
    batch = synth(S=4, n=40, L=12, F=T, box=80.0, seed=31, mixed_source=True)
    model, cfg = H.build_model(K, T, 0.5, init_seed=6)
    model = model.to(dev).eval()
    data = batch.to(dev)
    gf = runtime.GraphedForward(model, data)
    keys = ("loc", "pi", "diff_in", "diff_out")
    for seed in (5, 77):
        got = {k: gf(seed=seed)[k].clone() for k in keys}
        ref = batch.to(dev)
        with torch.no_grad():
            want = model(ref, noise=NoiseSpec(seed=seed))
        for k in keys:
            assert torch.equal(got[k], want[k]), (seed, k)
    a = gf(seed=5)["loc"].clone()
    assert not torch.equal(a, gf(seed=6)["loc"])
    # an edited batch (same shapes, same addresses): one actor steps aside at the last observed step
    data["positions"][0, 20] += 3.0
    edited = H.clone_batch(batch)
    edited["positions"][0, 20] += 3.0
    got = gf(seed=5)["loc"].clone()
    with torch.no_grad():
        want = model(edited.to(dev), noise=NoiseSpec(seed=5))["loc"]
    assert torch.equal(got, want) and not torch.equal(got, a)


def test_radius_test_on_borderline_pairs_follows_torch_norm(dev):
    """pairs whose distance sits within an ulp of the radius: the three ways of forming dx^2 + dy^2 in float32 (two fma
    contraction orders, no contraction) disagree about them.  The kernel forms it like torch.norm does on the reference's
    side (fma(dy, dy, fl(dx * dx))), so the edge lists still equal the oracle's exactly"""
    import numpy as np
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    offs = np.array([[37.32516098022461, 33.26908874511719], [-35.689231872558594, -35.01826095581055],
                     [-33.735321044921875, -36.9043083190918], [2.910139560699463, -49.91523742675781],
                     [-48.656944274902344, -11.51093578338623], [-29.218093872070312, -40.57465744018555]], dtype=np.float32)
    K, T = 2, 5
    batch = synth(S=1, n=7, L=3, F=T, box=10.0, seed=5)
    pos = torch.zeros_like(batch["positions"])
    pos[1:7] = torch.from_numpy(offs)[:, None, :]                       # actor 0 at the origin, nobody moves
    batch["positions"] = pos
    batch["x"] = torch.zeros_like(batch["x"])
    batch["padding_mask"] = torch.zeros_like(batch["padding_mask"])
    batch["bos_mask"] = torch.zeros_like(batch["bos_mask"])
    batch["bos_mask"][:, 0] = True
    d = torch.norm(pos[1:7, 0] - pos[0:1, 0], dim=-1)
    assert 0 < int((d < 50.0).sum()) < 6                                 # the oracle's own test splits these pairs
    model, cfg = H.build_model(K, T, 0.5, init_seed=2)
    want = H.oracle_forward(model, cfg, batch, noise_seed=3)
    model = model.to(dev)
    model.encoder.capture_intermediates = True
    model(batch.to(dev), noise=NoiseSpec(seed=3))
    im = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.encoder.last_intermediates.items()}
    Nt = batch.num_nodes + batch["agent_index"].numel()
    t_of = torch.div(im["aa_dst"], Nt, rounding_mode="floor")
    assert torch.equal(_sorted_cols(t_of * Nt + im["aa_src"], im["aa_dst"]), _sorted_cols(*want["aa_edge_list"]))


def test_relative_pose_prefetch_on_a_side_stream_is_bitwise_the_default_forward(dev):
    """runtime.arm_rel_prefetch / launch_rel_prefetch (TRAJSDE_OVERLAP_REL=1; C-ABI trajsde_encoder_fork_stream,
    trajsde_aggregator_prepare, trajsde_aggregator_forward_prepared): the aggregator's relative-pose embedding (AGG:42-51) on a
    side stream forked where the encoder's recurrence starts -- the same kernels on the same inputs, so the same bits, also
    when the forwards of two batches alternate (workspaces handed between the streams of the caching allocator)."""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import synth
    model, cfg = H.build_model(6, 20, 2.0, init_seed=2)
    model = model.to(dev)
    batches = [synth(S=6, n=40, L=12, F=20, box=120.0, seed=s, mixed_source=True) for s in (3, 4)]
    want = [{k: v.clone() for k, v in model(H.clone_batch(b).to(dev), noise=NoiseSpec(seed=9 + i)).items()} for i, b in enumerate(batches)]
    prev = runtime._OVERLAP_REL
    runtime._OVERLAP_REL = True
    try:
        for rep in range(3):
            for i, b in enumerate(batches):
                got = model(H.clone_batch(b).to(dev), noise=NoiseSpec(seed=9 + i))
                for k in ("loc", "pi", "diff_in", "diff_out"):
                    assert torch.equal(got[k], want[i][k]), (rep, i, k)
        torch.cuda.synchronize()
    finally:
        runtime._OVERLAP_REL = prev


# ----------------------------------------------------------------------------- irregular observation masks (synth.irregular_masks)
def test_graph_replay_under_irregular_masks_is_the_eager_forward(dev):
    """runtime.GraphedForward on a batch with gaps, rows padded at step 20 and rows never observed: bit for bit the eager forward"""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import irregular
    K, T = 3, 6
    batch = irregular(S=3, n=13, L=6, F=T, box=60.0, seed=36, mixed_source=True)
    model, cfg = H.build_model(K, T, 0.5, init_seed=6)
    model = model.to(dev).eval()
    gf = runtime.GraphedForward(model, batch.to(dev))
    keys = ("loc", "pi", "diff_in", "diff_out")
    for seed in (5, 77):
        got = {k: gf(seed=seed)[k].clone() for k in keys}
        with torch.no_grad():
            want = model(batch.to(dev), noise=NoiseSpec(seed=seed))
        for k in keys:
            assert torch.equal(got[k], want[k]), (seed, k)
            assert bool(torch.isfinite(got[k]).all()), k


def test_scene_run_alone_under_irregular_masks_gives_the_same_rows(dev):
    """test_scene_independence_and_sharding_invariance on irregular masks: the second scene of a two-scene batch run alone with the
    same global Philox row ids (same bound, 1e-5) -- its rows padded at step 20 and its never-observed rows included"""
    from trajsde_amd.data import collate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.synth import irregular_masks, synth
    K, T = 3, 5
    model, cfg = H.build_model(K, T, 0.5, init_seed=9)
    model = model.to(dev)
    a = synth(S=1, n=13, L=4, F=T, box=60.0, seed=37)
    b = synth(S=1, n=22, L=6, F=T, box=60.0, seed=38, source=1)
    both = irregular_masks(collate([a, b]), 39, T)
    na, nb = a.num_nodes, b.num_nodes
    for k in ("padding_mask", "bos_mask", "x"):
        b[k] = both[k][na:].clone()
    assert int(b["padding_mask"][:, 20].sum()) >= 4 and int((~b["bos_mask"].any(1)).sum()) >= 2

    def ids(lo, hi):
        return torch.arange(lo, hi, dtype=torch.int32, device=dev)

    tot = na + nb
    full = NoiseSpec(seed=77, fake_row_ids=ids(0, 2), enc_row_ids=torch.cat([ids(0, tot), ids(tot, tot + 2)]),
                     dec_row_ids=torch.cat([ids(k * tot, (k + 1) * tot) for k in range(K)]))
    part = NoiseSpec(seed=77, fake_row_ids=ids(1, 2), enc_row_ids=torch.cat([ids(na, tot), ids(tot + 1, tot + 2)]),
                     dec_row_ids=torch.cat([ids(k * tot + na, (k + 1) * tot) for k in range(K)]))
    with torch.no_grad():
        o2 = model(both.to(dev), noise=full)
        o1 = model(b.to(dev), noise=part)
    assert bool(torch.isfinite(o2["loc"]).all()) and bool(torch.isfinite(o1["loc"]).all())
    assert H.maxdiff(o2["loc"][:, na:].cpu(), o1["loc"].cpu()) <= 1e-5
    assert H.maxdiff(o2["pi"][na:].cpu(), o1["pi"].cpu()) <= 1e-5
    assert H.maxdiff(o2["diff_in"][1:].cpu(), o1["diff_in"].cpu()) <= 1e-5 and H.maxdiff(o2["diff_out"][1:].cpu(), o1["diff_out"].cpu()) <= 1e-5
