"""Whole full-size batches (-m gpu) against the float64 oracle run on the GPU.

The other oracle comparisons run on a few scenes of 1 to 257 actors, and the full-size tests (test_gpu_parity._full_size_properties,
test_gpu_backward's training-step cross-check) compare the kernels with themselves, or one scene of the batch with the oracle.  The
paths that only matter at size -- the weight-gradient reductions over millions of rows (k_wgrad6, k_wgrad6_edge), the deferred sums
and their areas, the cooperative recurrence over hundreds of tiles, the scene-cached global attention over 32 full scenes, the
gathering global attention and the split, merged CSR segments on 1024-actor scenes, the XCD dealing of workgroups -- meet a
reference only here.  oracle/restate.py follows the device of its inputs, so it runs in float64 on the GPU on the whole batch.

First the GPU oracle itself is checked against the CPU oracle (float64 and float32) on a small trained-weights case.  Then each
full-size case compares the whole batch with the float64 GPU oracle under the bounds of the small-batch tests: the forward's
outputs to TOL (test_gpu_trained_weights), every reached gradient of a training step through helpers.compare_grads (BACKWARD_REL of
each tensor's max, key biases under KEY_BIAS_ABS, widened only to 2 x the float32 GPU oracle's own deviation).  Each case prints its
worst error, its GPU time and its peak memory ("[full-size] ...")."""
import contextlib
import gc
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4
KEYS = ("loc", "pi", "diff_in", "diff_out")
SEED = 6
CHILD = os.path.join(H.ROOT, "tests", "grad_digest_child.py")
TIGHT = {"TRAJSDE_REDUCE_CAP": "600", "TRAJSDE_VPART_ARENA": "300000"}     # the deferred sums summed early, many times per entry point
EXACT = {"TRAJSDE_WGRAD_F32": "1", "TRAJSDE_IMMEDIATE_SUMS": "1", "TRAJSDE_RECUR_LEGACY": "1", "TRAJSDE_ROWS_BWD_MM": "0",
         "TRAJSDE_WGRAD_EDGE_PAIR": "0", "TRAJSDE_ROWS_BWD_FUSEW": "0", "TRAJSDE_REPLAY_COOP": "0", "TRAJSDE_SWEEP_COOP": "0"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def exact_fp32_matmul():
    """the float32 oracle on the GPU multiplies in fp32 (no TF32), as on the host"""
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _cost(tag):
    """prints the GPU time and the peak memory of the block"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"[full-size] {tag}: {time.perf_counter() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


@contextlib.contextmanager
def _fixed_order():
    """the oracle's scatter sums (index_add_ and its kin) in a fixed order on the GPU: the same float32 result on every run"""
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _scaled(a, ref):
    """max-abs error over max(1, max|ref|) (test_gpu_trained_weights._scaled)"""
    return H.maxdiff(a, ref) / max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ the GPU oracle against the CPU oracle
def _oracle_forward(model, cfg, batch, dt, device, drop):
    import restate
    P = {k: (v.detach().to(device, dt) if v.is_floating_point() else v.detach().to(device)) for k, v in model.state_dict().items()}
    return restate.forward(P, cfg, H.batch_as(batch, dt, device), H.NoiseAs(restate.PhiloxNoise(H.TRAINED_STEP_SEED), dt), drop=drop)


def _same(tag, got, want, rel, key_abs):
    """{name: max|got - want| / max|want|} over `want`'s tensors; key biases (zero in exact arithmetic) both under `key_abs`"""
    bad, worst = [], (0.0, "-")
    for k, w in want.items():
        g = got[k]
        if w is None or g is None:
            if (w is None) != (g is None):
                bad.append((k, "gradient on one side only"))
            continue
        g, w = g.detach().cpu().double(), w.detach().cpu().double()
        err, scale = H.maxdiff(g, w), float(w.abs().max()) if w.numel() else 0.0
        if H.zero_by_softmax_symmetry(k):
            if scale > key_abs or float(g.abs().max()) > key_abs:
                bad.append((k, err, scale))
        else:
            worst = max(worst, (err / max(scale, 1e-300), k))
            if err > rel * scale:
                bad.append((k, err, scale))
    print(f"[full-size] {tag}: worst {worst[1]} {worst[0]:.2e} of its max; {len(want)} tensors, {len(bad)} over")
    return bad


@pytest.mark.parametrize("mode", ["eval", "dropout"])
@pytest.mark.parametrize("dt,rel,key_abs", [(torch.float64, 1e-12, 1e-10), (torch.float32, 1e-5, H.KEY_BIAS_ABS)])
def test_gpu_oracle_matches_cpu_oracle(dt, rel, key_abs, mode, dev):
    """mixed_k6_t20 at strength 2: the forward's outputs and every gradient of the oracle's training step, on the GPU and on the
    host in the same dtype, to `rel` of each tensor's largest entry.  float64 measures 1.5e-14 at worst on MI355X.  float32 measures
    1.1e-6 (pi) and 6.0e-6 (gradients): another summation order in every product and reduction, through the 21-step recurrences --
    the float32 oracle serves only as the noise32 widening, a hundred times below BACKWARD_REL"""
    model, cfg, batch, kw = H.trained_step_case("mixed_k6_t20", mode, 2.0)
    drop = kw.get("drop")
    with _fixed_order():
        outs = [_oracle_forward(model, cfg, batch, dt, d, drop) for d in ("cpu", dev)]
    assert all(outs[1][k].device.type == "cuda" and outs[1][k].dtype == dt for k in KEYS)
    bad = _same(f"oracle forward {mode} {dt}", outs[1], {k: outs[0][k] for k in KEYS}, rel, key_abs)
    assert torch.equal(outs[0]["reg_mask"], outs[1]["reg_mask"].cpu())
    with _fixed_order():
        steps = [H.oracle_full_grads(model, cfg, batch, H.TRAINED_STEP_SEED, 1.0, 0.5, dt=dt, device=d, **kw) for d in ("cpu", dev)]
    (loss_cpu, want), (loss_gpu, got) = steps
    assert abs(loss_gpu - loss_cpu) <= rel * max(1.0, abs(loss_cpu))
    assert all(g is None or g.device.type == "cuda" for g in got.values())
    bad += _same(f"oracle gradients {mode} {dt}", got, want, rel, key_abs)
    assert not bad, bad


# ------------------------------------------------------------------ forward
FORWARD_CASES = [("metric256", 0.0, "injected"), ("metric256", 1.0, "injected"), ("metric256", 2.0, "injected"),
                 ("metric256", 1.0, "philox"), ("config3", 1.0, "injected"), ("config5", 1.0, "injected")]


def _forward_noise(name, batch, cfg, kind, dev):
    """(NoiseSpec for the kernels, restate noise source for the oracle): the same normals on both sides -- drawn on the device and
    injected (z_fake / z_enc / z_dec), or the in-kernel Philox stream over global row ids (shard.global_noise_spec) and its host twin"""
    import restate
    from trajsde_amd.runtime import NoiseSpec
    from trajsde_amd.schedule import decoder_schedule
    from trajsde_amd.shard import global_noise_spec
    c = restate.flat_cfg(cfg)
    K, N, A, Hs = c["num_modes"], batch.num_nodes, batch["agent_index"].numel(), c["historical_steps"]
    if kind == "philox":
        counts = torch.bincount(batch["batch"]).tolist()
        ns = global_noise_spec(SEED, range(len(counts)), counts, K, device=dev)
        return ns, restate.PhiloxNoise(SEED, enc_row_ids=ns.enc_row_ids.cpu().numpy(), dec_row_ids=ns.dec_row_ids.cpu().numpy(),
                                       fake_row_ids=ns.fake_row_ids.cpu().numpy())
    n_euler = decoder_schedule(c["future_steps"], c["max_fut_t"], c["min_stepsize"]).n_euler
    g = torch.Generator(device=dev).manual_seed(SEED)
    z_fake = torch.randn(A, Hs, 2, generator=g, device=dev)
    z_enc = torch.randn(Hs, N + A, 64, generator=g, device=dev)
    z_dec = torch.randn(n_euler, K * N, 64, generator=g, device=dev)
    return NoiseSpec(seed=0, z_fake=z_fake, z_enc=z_enc, z_dec=z_dec), restate.InjectedNoise(z_fake, z_enc, z_dec)


def _per_scene(o, want, batch):
    """the worst error of loc / pi / diff_in / diff_out in each scene"""
    scene = batch["batch"].to(o["loc"].device)
    S = int(scene.max()) + 1
    e_actor = torch.maximum((o["loc"].double() - want["loc"]).abs().amax(dim=(0, 2, 3)), (o["pi"].double() - want["pi"]).abs().amax(1))
    worst = torch.zeros(S, dtype=torch.float64, device=e_actor.device).scatter_reduce(0, scene, e_actor, "amax")
    agent_scene = scene[batch["agent_index"].to(scene.device)]
    for k in ("diff_in", "diff_out"):
        e = (o[k].double() - want[k]).abs().reshape(agent_scene.numel(), -1).amax(1)
        worst = worst.scatter_reduce(0, agent_scene, e, "amax")
    return worst.cpu().tolist()


@pytest.mark.parametrize("name,strength,noise_kind", FORWARD_CASES)
def test_full_size_forward_matches_float64_gpu_oracle(name, strength, noise_kind, dev):
    """the whole batch: loc, pi, diff_in, diff_out to TOL; local_embed from the encoder stage and global_embed from the aggregator
    stage fed the oracle's local_embed, to TOL of max(1, max|oracle|) (test_stages_in_isolation_match_float64_oracle)"""
    import restate
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    from trajsde_amd.runtime import rotate_inputs
    from trajsde_amd.synth import CONFIGS, synth
    spec = CONFIGS[name]
    cfg = H.our_cfg(spec["num_modes"], spec["future_steps"], spec["max_fut_t"])
    model = PredictionModelSDENet(**cfg, init_seed=0).eval()
    if strength:
        H.trained_like_parameters(model, H.TRAINED_SEED, strength)
    batch = synth(**spec["synth"])
    tag = f"{name} s={strength} {noise_kind}"
    ns, src = _forward_noise(name, batch, cfg, noise_kind, dev)
    with _cost(f"float64 oracle forward {tag}"):
        want = H.oracle_forward64(model, cfg, batch, noise=src, device=dev)
    model = model.to(dev)
    with _cost(f"kernels forward {tag}"), torch.no_grad():
        o = model(H.clone_batch(batch).to(dev), noise=ns)
    _check_range()
    errs = {k: H.maxdiff(o[k], want[k]) for k in KEYS}
    assert torch.equal(o["reg_mask"], want["reg_mask"])
    worst = _per_scene(o, want, batch)
    del o
    data = H.clone_batch(batch).to(dev)
    data["rotate_mat"], _ = rotate_inputs(data)
    c = restate.flat_cfg(cfg)
    P = {k: (v.detach().double() if v.is_floating_point() else v.detach()) for k, v in model.state_dict().items()}
    b64 = H.batch_as(batch, torch.float64, dev)
    rot64, _ = restate.rotate_inputs(b64)
    with torch.no_grad():
        local, *_ = model.encoder(data=data, noise=ns)
        errs["local_embed"] = _scaled(local, want["local_embed"])
        local32 = want["local_embed"].float()
        g = model.aggregator(data=data, local_embed=local32)
        errs["global_embed"] = _scaled(g, restate.global_interactor(P, c, b64, rot64, local32.double()))
    _check_range()
    print(f"[full-size] forward {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"[full-size] forward {tag}: worst per scene " + " ".join(f"{v:.1e}" for v in worst))
    del want, local, g, P, b64, data
    _free()
    for k, e in errs.items():
        assert e <= TOL, (k, e)


def _check_range():
    from trajsde_amd import _lib
    torch.cuda.synchronize()
    _lib.check_range()                           # no fp16x3 operand left the fp16 range on the way


# ------------------------------------------------------------------ training step
def _child_args(name, mode, strength):
    args = [name]
    if strength:
        args += ["--strength", str(strength)]
    if mode != "train":
        args.append("--eval")
    if mode == "nll":
        args.append("--nll")
    return args


def _run_child(args, env_extra, dump):
    """the step in a child process (grad_digest_child.py): (loss, {param: gradient})"""
    env = dict(os.environ, TRAJSDE_TEST_DUMP=str(dump), **env_extra)
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, CHILD, *args], env=env, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    print(f"[full-size] kernels step {' '.join(args)} {env_extra or 'default forms'}: {time.perf_counter() - t0:.1f} s (child process)")
    return json.loads(r.stdout.strip().splitlines()[-1])["loss"], torch.load(dump)


# (configuration, mode, strength, kernel forms): "train" is train mode with the YAML's dropout 0.1, "nll" the Laplace NLL in eval mode;
# "exact": the forms test_full_size_training_step_agrees_between_kernel_forms compares with (exact fp32 weight-gradient products,
# immediate sums, the legacy recurrence and sweeps)
STEP_CASES = [("config2", "eval", 0.0, ("default", "tight")), ("config2", "train", 0.0, ("default", "tight")),
              ("config2", "eval", 1.0, ("default", "tight")), ("config2", "train", 1.0, ("default", "tight", "exact")),
              ("config2", "nll", 1.0, ("default",)), ("config4", "train", 0.0, ("default",))]

# Gradients over BACKWARD_REL at full size, measured on MI355X (every kernel form alike), kept out of the main test and asserted in
# test_full_size_training_step_known_excess, which is expected to fail.  (Not listed: in train mode at strength 1 a dozen gradients
# whose sums over the batch cancel -- the AL lane embedding, the global rel embedding, the first global layer's gate, the decoder's
# input LayerNorm -- land 2.1e-4 .. 4.1e-4 of their max, within 2 x the float32 oracle's own deviation, i.e. inside the noise32
# widening; the exact fp32 kernel forms measure the same, 3.9e-4 on lane_embed.module_list.1.0.weight.)
_FFN0 = ("aggregator.global_interactor_layers.0.mlp.0.weight", "aggregator.global_interactor_layers.0.mlp.0.bias")
KNOWN_EXCESS = {
    # 2.8e-4 / 3.0e-4 (train, initial weights) and 2.5e-4 / 2.4e-4 (eval, strength 1) of the tensors' max, where the float32 oracle
    # lands 1e-6 of it: the weight and the bias of ONE ReLU layer move together, by the size of one row's term -- among the 8192 x 256
    # hidden units of the first global layer's FFN a few lie within the kernels' forward rounding of zero, and a unit on the other side
    # of its kink adds or drops its whole contribution (test_gpu_trained_backward._away_from_relu_kinks, at small size)
    ("config2", "train", 0.0): (_FFN0, "layers.0.mlp.0 weight / bias 3.0e-4 / 2.8e-4 of their max (float32 oracle 2e-6): ReLU units "
                                       "of the first global FFN within the kernels' forward rounding of their kink"),
    ("config2", "eval", 1.0): (_FFN0, "layers.0.mlp.0 weight / bias 2.4e-4 / 2.5e-4 of their max (float32 oracle 1e-6): ReLU units "
                                      "of the first global FFN within the kernels' forward rounding of their kink"),
}
_STEP = {}


def _step(name, mode, strength, forms, dev, tmp_path):
    """(kernel results {form: (loss, grads)}, float64 loss, float64 grads on the host, noise32, the names float64 says are reached),
    computed once per case: the step in child processes, then float64 and float32 autograd over the oracle on the GPU"""
    key = (name, mode, strength)
    if key in _STEP:
        return _STEP[key]
    import grad_digest_child as C
    import restate
    from trajsde_amd.synth import synth
    args = _child_args(name, mode, strength)
    _free()
    results = {f: _run_child(args, {"tight": TIGHT, "exact": EXACT}.get(f, {}), tmp_path / f"{f}.pt") for f in forms}
    model, cfg, spec = C.step_model(args, "cpu")
    batch = synth(**spec["synth"])
    w_l2, w_diff = (float(w) for w in model.loss_weights)
    kw = dict(drop=restate.PhiloxDropout(C.DROPOUT_SEED, float(cfg["encoder"]["kwargs"]["dropout"])) if mode == "train" else None,
              nll_eps=1e-6 if mode == "nll" else None)
    tag = f"{name} {mode} s={strength}"
    with _cost(f"float64 oracle step {tag}"):
        want_loss, want = H.oracle_full_grads(model, cfg, batch, C.NOISE_SEED, w_l2, w_diff, device=dev, **kw)
    _free()
    # the float32 oracle's own deviation widens bounds (noise32): one number per tensor, not a new draw of atomics on every run
    with _fixed_order(), _cost(f"float32 oracle step {tag}"):
        _, want32 = H.oracle_full_grads(model, cfg, batch, C.NOISE_SEED, w_l2, w_diff, dt=torch.float32, device=dev, **kw)
    noise32 = H.deviation(want32, want)
    del want32
    want = {k: (w.cpu() if w is not None else None) for k, w in want.items()}
    _free()
    nonzero = {n for n, _ in model.named_parameters() if want.get(n) is not None and float(want[n].abs().max()) > 0}
    _STEP[key] = (results, want_loss, want, noise32, nonzero)
    return _STEP[key]


@pytest.mark.parametrize("name,mode,strength,forms", STEP_CASES)
def test_full_size_training_step_matches_float64_gpu_oracle(name, mode, strength, forms, dev, tmp_path):
    """the whole batch's training step, in the default kernel forms and with the deferred sums' areas tight (TRAJSDE_REDUCE_CAP /
    TRAJSDE_VPART_ARENA), against float64 autograd over the oracle on the GPU with the same Philox noise and dropout masks: the loss
    to 1e-5 relative (2e-5 under the NLL, as at small size), the reached set, every gradient but the case's KNOWN_EXCESS through
    helpers.compare_grads"""
    results, want_loss, want, noise32, nonzero = _step(name, mode, strength, forms, dev, tmp_path)
    known = set(KNOWN_EXCESS.get((name, mode, strength), ((), ""))[0])
    tag = f"{name} {mode} s={strength}"
    loss_tol = 2e-5 if mode == "nll" else 1e-5
    bad = []
    for form, (loss, grads) in results.items():
        print(f"[full-size] step {tag} {form}: loss {loss:.9g}, float64 oracle {want_loss:.9g}")
        if abs(loss - want_loss) > loss_tol * max(1.0, abs(want_loss)):
            bad.append((form, "loss", loss, want_loss))
        if set(grads) != nonzero:
            bad.append((form, "reached", sorted(set(grads) ^ nonzero)[:6]))
        over = H.compare_grads(f"full-size step {tag} {form}", {k: g for k, g in grads.items() if k not in known}, want, noise32=noise32)
        for b in over:
            print(f"[full-size] over {tag} {form}: {b[0]} {b[1] / b[2]:.2e} of its max ({b[1]:.2e}), float32 oracle {b[3]:.2e}")
        bad += [(form,) + b for b in over]
    assert not bad, bad[:8]


@pytest.mark.parametrize("name,mode,strength,forms", [
    pytest.param(*case, marks=pytest.mark.xfail(strict=True, reason=KNOWN_EXCESS[case[:3]][1])) for case in STEP_CASES
    if case[:3] in KNOWN_EXCESS])
def test_full_size_training_step_known_excess(name, mode, strength, forms, dev, tmp_path):
    """the gradients KNOWN_EXCESS keeps out of the test above, under the same rule"""
    results, _, want, noise32, _ = _step(name, mode, strength, forms, dev, tmp_path)
    known = set(KNOWN_EXCESS[(name, mode, strength)][0])
    bad = []
    for form, (_, grads) in results.items():
        over = H.compare_grads(f"full-size step {name} {mode} s={strength} {form}, known excess",
                               {k: g for k, g in grads.items() if k in known}, want, noise32=noise32)
        for b in over:
            print(f"[full-size] over {name} {mode} s={strength} {form}: {b[0]} {b[1] / b[2]:.2e} of its max ({b[1]:.2e}), "
                  f"float32 oracle {b[3]:.2e}")
        bad += over
    assert not bad, bad[:8]
