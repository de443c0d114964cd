"""Where the kernels read and write memory (-m gpu): every launch entry point of include/trajsde_hip.h run with its inputs, outputs and
workspaces inside red-zone arenas (tests/guarded_memory.py), at the shapes where tiles are partial or empty.

The header's contract: every entry point "BORROWS its pointers" and "writes only into caller-provided buffers", workspace sizes come from
the *_ws_bytes queries, inputs are const.  For every case the same call runs under several fills, and
  (a) no guard byte of any arena is touched and no input changes;
  (b) the outputs are finite when every workspace and output starts as NaN;
  (c) the outputs are bit-identical across fills: input guards NaN / 0 / 0 against 1e30 / 1 / 1 (nothing read out of bounds reaches a
      result), interiors NaN against zero against random bits (nothing uninitialised reaches a result).  No tolerance: every launch is
      bit-reproducible (README).  The one documented exception is the atomic scatter the aggregator backward takes for an asymmetric
      input graph: the training steps of such cases assert (a) and (b) only.
Buffers the header tells the caller to pre-zero (`grads` of the encoder, aggregator and grid backwards) are zeroed as the header says
(runtime.StageRuntime._grad_buffers uses torch.zeros); nothing else is.

The interception cannot lapse silently: every test asserts that the pointers the library received -- the fields of gc.batch, the graph
workspaces, the rotation, the outputs -- lie inside arenas.  What the guards cannot see is listed in tests/guarded_memory.py (jumps past
the guard, masked reads, overruns inside a workspace); inputs that torch itself allocates inside the runtime (the step tables, reg_mask,
the sum of two d_local tensors) are not in arenas, so an overread of those is not seen either."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded_memory as GM
import helpers as H

pytestmark = pytest.mark.gpu
SEED = 6
STRENGTH = H.TRAINED_STRENGTHS[0]
FILL_RUNS = (("A", "nan"), ("B", "nan"), ("A", "zero"), ("A", 7))        # (input-guard fill, interior poison); the first is the baseline
BATCH_FIELDS = ("x", "positions", "padding_mask", "bos_mask", "rotate_angles", "edge_index", "agent_index", "batch", "source",
                "lane_positions", "lane_paddings", "lane_actor_index", "lane_actor_vectors")
CALLED, RAN, COUNTS = set(), set(), []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    spy_on_library()
    return torch.device("cuda:0")


def spy_on_library():
    """every entry of _lib.SIGNATURES notes its name in CALLED when it is called (the coverage table at the end of this module)"""
    from trajsde_amd import _lib
    L = _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    if getattr(L, "_memory_contract_spy", False):
        return

    def wrap(name, fn):
        def spy(*a):
            CALLED.add(name)
            return fn(*a)
        return spy
    for name in _lib.SIGNATURES:
        setattr(L, name, wrap(name, getattr(L, name)))
    L._memory_contract_spy = True


# ----------------------------------------------------------------------------------------------------------------- batches
def _trim_edges(ei, target, symmetric):
    """the first `target` columns (an asymmetric list), or the list without its last (E - target) / 2 actor pairs, both directions"""
    drop = ei.shape[1] - target
    assert drop >= 0
    if drop == 0:
        return ei
    if not symmetric:
        return ei[:, :target].clone()
    assert drop % 2 == 0
    key = torch.minimum(ei[0], ei[1]) * (1 << 20) + torch.maximum(ei[0], ei[1])
    return ei[:, ~torch.isin(key, key.unique()[-(drop // 2):])].clone()


def shape_case(ns, seed, T, e_res=None, la_res=None, symmetric=True):
    """scenes of `ns` agents (box 30 m: every lane within the 50 m radius, agent pairs drift apart over the history), 30 % of the
    actors with a late first observation; `e_res` / `la_res`: the edge list cut to the largest length = e_res mod 64, all but the first
    (largest count = la_res mod 64) lane-actor pairs moved beyond the radius"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    b = collate([synth(S=1, n=n, L=4, F=T, box=30.0, seed=100 * seed + i, history_dropout=0.3, source=i % 2) for i, n in enumerate(ns)])
    if e_res is not None:
        E = b["edge_index"].shape[1]
        b["edge_index"] = _trim_edges(b["edge_index"], E - (E - e_res) % 64, symmetric)
    if la_res is not None:
        n_la = b["lane_actor_index"].shape[1]
        v = b["lane_actor_vectors"].clone()
        v[n_la - (n_la - la_res) % 64:] += 1000.0
        b["lane_actor_vectors"] = v
    return b


# name -> (agents per scene, seed, K, T, edge-count residue, symmetric, lane-pair residue, training variant).  Row counts one below, at and
# one above multiples of 16 AND of 64 (63, 64, 65 are -1, 0, +1 of both): N = 63 / 64 / 65 (with K = 1 also K*N), Nt = N + A = 63 / 64 /
# 65, H*Nt = 21 * 67 / 21 * 64 / 21 * 61 = 63 / 0 / 1 mod 64, E_g = E = 63 / 0 / 1 mod 64 (an odd list cannot be symmetric), E_la by
# construction, E_aa (data dependent) by the choice of the seeds.  test_zz_row_counts_reach_every_residue_class asserts what was reached.
SHAPE_CASES = {
    "n63_k1_t12": ((21, 21, 21), 2, 1, 12, None, True, 63, "l2"),
    "n64_k1_t30": ((21, 21, 22), 7, 1, 30, 0, True, 0, "nll"),
    "n65_k1_t60": ((21, 22, 22), 1, 1, 60, None, True, 1, "milstein"),
    "nt63_k6_t30": ((20, 20, 20), 1, 6, 30, 63, False, None, "l2"),
    "nt64_k10_t60": ((20, 20, 21), 1, 10, 60, None, True, None, "milstein_nll"),
    "nt65_k6_t12": ((20, 21, 21), 1, 6, 12, 1, False, None, "nll"),
    "nt61_k10_t12": ((20, 20, 18), 1, 10, 12, None, True, None, "l2"),
}


def _case_batch(name):
    ns, seed, K, T, e_res, sym, la_res, _ = SHAPE_CASES[name]
    return shape_case(ns, seed, T, e_res, la_res, sym)


def degenerate_batch(name, T):
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    if name == "single":                                             # one scene with one agent
        return synth(S=1, n=1, L=2, F=T, box=30.0, seed=60)
    if name == "lonely":                                             # E = 0
        return collate([synth(S=1, n=1, L=2, F=T, box=30.0, seed=60 + i) for i in range(3)])
    if name == "far":                                                # E_la = 0
        b = synth(S=2, n=5, L=3, F=T, box=40.0, seed=70)
        b["lane_actor_vectors"] = b["lane_actor_vectors"] + 1000.0
        return b
    if name == "dup":                                                # repeated edges (count twice; the list is no longer symmetric)
        b = synth(S=1, n=6, L=3, F=T, box=40.0, seed=71)
        ei = torch.cat([b["edge_index"], b["edge_index"][:, :7]], dim=1)
        b["edge_index"] = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(3))]
        return b
    if name == "padded":                                             # all history padded for some actors: only the current step is there
        b = synth(S=2, n=8, L=3, F=T, box=40.0, seed=74, history_dropout=0.3)
        for i in (1, 9, 15):
            b["padding_mask"][i, :20] = True
            b["bos_mask"][i] = False
            b["bos_mask"][i, 20] = True
            b["x"][i] = 0.0
        return b
    if name == "isolated":
        return H._isolated_batch(T)
    if name == "nolanes":                                            # L = 0 with E_al = 0
        b = synth(S=2, n=6, L=0, F=T, box=40.0, seed=75)
        assert b["lane_positions"].shape[0] == 0 and b["lane_actor_index"].shape[1] == 0
        return b
    raise KeyError(name)


DEGENERATE = ("single", "lonely", "far", "dup", "padded", "isolated", "nolanes")
ASYMMETRIC = {"dup", "nt63_k6_t30", "nt65_k6_t12"}                  # their aggregator backward scatters with float atomics


# ----------------------------------------------------------------------------------------------------------------- models
def sde_model(K, T, variant="l2", dropout=None):
    """the SDE model at trained-like weights; `variant`: l2 | nll | milstein | milstein_nll (regression loss, decoder solver)"""
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T, T / 10.0)
    if "nll" in variant:
        cfg["losses_module"] = ["LaplaceNLLLoss", "DiffBCE"]
        cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"}, {"reduction": "mean"}]
    if "milstein" in variant:
        cfg["decoder"]["kwargs"]["method"] = cfg["encoder"]["kwargs"]["method"] = "milstein"
    if dropout is not None:
        cfg["encoder"]["kwargs"]["dropout"] = cfg["aggregator"]["kwargs"]["dropout"] = dropout
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    model.loss_weights = [1.0, 0.5]
    H.trained_like_parameters(model, H.TRAINED_SEED, STRENGTH)
    return model


def grid_model(K, T, heads=4, layers=2, nll=False, dropout=0.1):
    from trajsde_amd.models.model_base_mix import PredictionModel
    cfg = H.grid_cfg(K, T, heads, layers, dropout=dropout)
    if nll:
        cfg["losses_module"] = ["LaplaceNLLLoss"]
        cfg["loss_args"] = [{"eps": 1e-6, "reduction": "mean"}]
    model = PredictionModel(**cfg, init_seed=9).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, STRENGTH)
    return model


# ----------------------------------------------------------------------------------------------------------------- the harness
def place_batch(gm, batch, fill):
    """the batch with every field the C-ABI reads inside an arena, in the dtype GraphContext.f32 / u8 / i64 expect (so that they hand
    the placed storage itself to the library).  Index guards hold 0 / 1 only where both are valid ids (N >= 2, and L >= 2 unless no
    lane index is read); elsewhere they hold 0 under both fills."""
    from trajsde_amd.data import TemporalData
    N, L, E_al = batch["x"].shape[0], batch["lane_positions"].shape[0], batch["lane_actor_index"].shape[1]
    ids_ok = N >= 2 and (L >= 2 or E_al == 0)
    out = TemporalData(**batch.as_dict())
    for k in BATCH_FIELDS + (("y",) if batch.y is not None else ()):
        t = batch[k]
        if t.is_floating_point():
            t = t.to(torch.float32)
        out[k] = gm.placed(t, fill if (ids_ok or t.dtype != torch.int64) else "A", label=k)
    return out


def assert_graph_pointers(gm, data, fake_agents=True):
    """the library really received arena memory: the batch fields are the placed tensors, the graph stage's buffers are arenas"""
    from trajsde_amd.runtime import GraphContext
    gc = data[GraphContext.KEY]
    for k in BATCH_FIELDS:
        t = data[k]
        want = (t.data_ptr() or None) if (t.numel() or t.dtype != torch.int64) else None
        if k == "agent_index" and not fake_agents:
            want = None
        assert getattr(gc.batch, k) == want, (k, getattr(gc.batch, k), want)
        assert want is None or gm.owns(t), k
    for name, t in (("ws", gc.ws), ("edges_ws", gc.edges_ws), ("rot", gc.rot)):
        assert t.numel() == 0 or gm.owns(t), name
    return gc


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def note_counts(tag, gc, K):
    c = gc.true_counts()
    b = gc.batch
    row = {"case": tag, "N": b.N, "Nt": gc.graph.Nt, "K*N": K * b.N, "H*Nt": b.H * gc.graph.Nt, "E": b.E, **c}
    if row not in COUNTS:
        COUNTS.append(row)
        print("[memory-contract] counts", json.dumps(row))


def contract(tag, make_inputs, call, compare=True, runs=FILL_RUNS):
    """`make_inputs(gm, fill)` -> the placed inputs, `call(inputs)` (run inside the routing context) -> (compared {name: tensor},
    tensors that must lie in arenas).  Asserts (a) and (b) for every run and (c) between the first run and each of the others."""
    base, n_arenas = None, 0
    for fill, poison in runs:
        gm = GM.GuardedMemory(poison=poison)
        inputs = make_inputs(gm, fill)
        with gm:
            outs, owned = call(inputs)
        torch.cuda.synchronize()
        where = f"{tag} [guards {fill}, poison {poison}]"
        assert gm.routed > 0, where
        for i, t in enumerate(owned):
            assert t.numel() == 0 or gm.owns(t), (where, "output not in an arena", i, tuple(t.shape))
        post = getattr(call, "after", None)
        if post is not None:
            post(gm, inputs)
        rep = gm.check()
        assert rep.ok, f"{where}\n{rep}"                                                       # (a)
        if poison == "nan":
            bad = [k for k, v in outs.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]
            assert not bad, (where, "non-finite", bad)                                         # (b)
        outs = {k: v.detach().clone() for k, v in outs.items()}
        n_arenas += rep.n_arenas
        if base is None:
            base = outs
        elif compare:
            assert outs.keys() == base.keys()
            diff = [k for k in outs if not torch.equal(_bits(outs[k]), _bits(base[k]))]
            assert not diff, (where, "differs from the first run", diff[:8], len(diff))        # (c)
    print(f"[memory-contract] {tag}: {len(runs)} runs, {n_arenas} arenas clean" + ("" if compare else " (asymmetric graph: (a) and (b) only)"))


FWD_KEYS = ("loc", "pi", "diff_in", "diff_out")


def forward_contract(tag, model, batch, dev, K, keys=FWD_KEYS, fake_agents=True, compare=True, extra=None, runs=FILL_RUNS):
    """model(batch) under the contract; `extra(model, data, out)` -> more compared tensors"""
    from trajsde_amd.runtime import NoiseSpec
    on_dev = batch.to(dev)

    def call(data):
        with torch.no_grad():
            out = model(data, noise=NoiseSpec(seed=SEED, dropout_seed=SEED + 1))
        outs = {k: out[k] for k in keys}
        if extra is not None:
            outs.update(extra(model, data, out))
        return outs, [out["loc"], out["pi"]] + [v for v in outs.values() if v.is_floating_point()]

    def after(gm, data):
        note_counts(tag, assert_graph_pointers(gm, data, fake_agents), K)
        assert data.y is None or gm.owns(data.y)                     # the rotated targets (runtime.rotate_inputs) are an output too
    call.after = after
    contract(tag, lambda gm, fill: place_batch(gm, on_dev, fill), call, compare=compare, runs=runs)


def training_contract(tag, model, batch, dev, K, compare=True, runs=FILL_RUNS):
    """model.training_step(batch).backward() under the contract: the loss and every gradient word"""
    from trajsde_amd.runtime import NoiseSpec
    on_dev = batch.to(dev)
    model.train()

    def call(data):
        for p in model.parameters():
            p.grad = None
        loss = model.training_step(data, 0, noise=NoiseSpec(seed=SEED, dropout_seed=SEED + 1))
        loss.backward()
        outs = {"loss": loss.detach().reshape(1)}
        outs.update({n: p.grad for n, p in model.named_parameters() if p.grad is not None})
        assert len(outs) > 50
        o = model.last_output
        return outs, [o["loc"] if o["loc"].shape[-1] == 4 else o["_loc4"], o["pi"]]

    def after(gm, data):
        note_counts(tag, assert_graph_pointers(gm, data, fake_agents=hasattr(model.encoder, "real_label")), K)
    call.after = after
    contract(tag, lambda gm, fill: place_batch(gm, on_dev, fill), call, compare=compare, runs=runs)
    model.eval()


# ----------------------------------------------------------------------------------------------------------------- the helper on the device
def test_planted_write_on_a_device_arena_is_reported(dev):
    """the self-test's planted one-byte writes on device arenas: torch indexing into the arena tensor (legal memory, no kernel)"""
    gm = GM.GuardedMemory(poison="nan")
    with gm:
        a = torch.empty(5, 64, device=dev, dtype=torch.float32)
        b = torch.zeros(33, device=dev, dtype=torch.uint8)
        host = torch.empty(4)
    p = gm.placed(torch.arange(6, device=dev).view(2, 3), "B")
    assert gm.owns(a) and gm.owns(b) and gm.owns(p) and not gm.owns(host) and gm.routed == 2
    assert a.data_ptr() % 512 == 0 and bool(torch.isnan(a).all()) and bool((b == 0).all())
    assert gm.check().ok
    G, ar = gm.guard, gm.arenas[1]
    for at, side, off in ((G + ar.nbytes, "tail", 0), (G - 1, "lead", -1), (G + ar.nbytes + G - 1, "tail", G - 1)):
        ar.mem[at] ^= 1
        torch.cuda.synchronize()
        rep = gm.check()
        assert len(rep.hits) == 1 and rep.hits[0][0] is ar and rep.hits[0][1:] == (side, off, 1), str(rep)
        assert "zeros(33,)" in str(rep) and "test_gpu_memory_contract.py" in str(rep)
        ar.mem[at] ^= 1
    p[0, 0] = 9
    rep = gm.check()
    assert not rep.hits and len(rep.changed) == 1 and rep.changed[0][0] is gm.arenas[2]


# ----------------------------------------------------------------------------------------------------------------- whole model, partial tiles
@pytest.mark.parametrize("name", list(SHAPE_CASES))
def test_inference_forward_at_partial_tile_shapes(name, dev):
    """trajsde_rotate, _graph_prepare_async, _graph_compact, _encoder_forward, _aggregator_forward_heads (8 heads), _decoder_forward
    (Euler and Milstein) through model(...), in the sync-free form (list lengths on the device, buffers sized from bounds)"""
    RAN.add("forward")
    ns, seed, K, T, _, _, _, variant = SHAPE_CASES[name]
    model = sde_model(K, T, "milstein" if "milstein" in variant else "l2").to(dev)
    forward_contract(f"forward {name}", model, _case_batch(name), dev, K)


@pytest.mark.parametrize("name", list(SHAPE_CASES))
def test_training_step_at_partial_tile_shapes(name, dev):
    """trajsde_graph_prepare, _pack_weights_many, _encoder_forward_train, _aggregator_forward_train, the four decoder backwards,
    _aggregator_backward_heads, _encoder_backward (tape + separate scratch) through model.training_step(...).backward() in train
    mode (dropout 0.1)"""
    RAN.add("training")
    ns, seed, K, T, _, _, _, variant = SHAPE_CASES[name]
    model = sde_model(K, T, variant).to(dev)
    training_contract(f"training[{variant}] {name}", model, _case_batch(name), dev, K, compare=name not in ASYMMETRIC)


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_graphs_forward_and_training(name, dev):
    """one agent, no edges, no lane within the radius, duplicated edges, actors without history, isolated targets, and no lanes at all
    (L = 0 with E_al = 0: the entry points accept it -- the lane arrays are then empty arenas whose guards meet)"""
    RAN.add("degenerate")
    K, T = 6, 12
    model = sde_model(K, T).to(dev)
    batch = degenerate_batch(name, T)
    forward_contract(f"forward {name}", model, batch, dev, K)
    training_contract(f"training {name}", model, batch, dev, K, compare=name not in ASYMMETRIC)


def test_capture_ood_and_exact_forward(dev):
    """trajsde_export_senders(1) + trajsde_graph_prepare (exact) + trajsde_encoder_forward with aa_out / latent_ys; the same batch with
    the synchronising graph stage and no capture; trajsde_encoder_forward_ood (A = 0: no fake agents)"""
    from trajsde_amd import runtime
    RAN.add("capture")
    K, T = 6, 12
    model = sde_model(K, T).to(dev)
    batch = _case_batch("nt61_k10_t12")
    model.encoder.capture_intermediates = True

    def inter(m, data, out):
        im = m.encoder.last_intermediates
        assert im["aa_src"].numel() == im["aa_dst"].numel() > 0 and im["la_lane"].numel() == im["la_dst"].numel() > 0
        return {k: im[k] for k in ("aa_out", "latent_ys", "aa_src", "aa_dst", "aa_segptr", "g_src", "g_dst", "la_lane", "la_dst")}
    forward_contract("forward, captured intermediates", model, batch, dev, K, extra=inter)
    model.encoder.capture_intermediates = False
    prev = runtime.set_sync_free(False)
    try:
        forward_contract("forward, exact graph", model, batch, dev, K)
    finally:
        runtime.set_sync_free(prev)
    model.ood = True
    for tag, b in (("mixed", batch), ("isolated", degenerate_batch("isolated", T))):
        forward_contract(f"forward_ood {tag}", model, b, dev, K, keys=("loc", "pi", "stds"), fake_agents=False)
    model.ood = False


def test_prepared_and_legacy_aggregator_entry_points(dev):
    """trajsde_aggregator_prepare (on a side stream) + _forward_prepared against _forward_heads, and the two entry points without a
    head count (trajsde_aggregator_forward / trajsde_aggregator_backward: 8 heads) through ctypes"""
    from trajsde_amd import _lib
    from trajsde_amd.runtime import D, GraphContext, NoiseSpec, rotate_inputs
    RAN.add("aggregator")
    K, T = 6, 12
    model = sde_model(K, T).to(dev)
    rt = model.aggregator._rt
    on_dev = _case_batch("nt65_k6_t12").to(dev)                       # an odd (asymmetric) global list: E_g = 1 mod 64
    L = _lib.lib()
    nl = int(model.aggregator.num_layers)

    def call(data):
        st = torch.cuda.current_stream().cuda_stream
        with torch.no_grad():
            data["rotate_mat"], _ = rotate_inputs(data)
            local = model.encoder(data=data, noise=NoiseSpec(seed=SEED))[0]
            plain = model.aggregator(data=data, local_embed=local, noise=None)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            prep = rt.launch_rel_prefetch(data, side)
            assert prep is not None
            prepared = model.aggregator(data=data, local_embed=local, noise=None, prepared=prep)
            gc = GraphContext.get(data, None, 21, None)
            N = gc.batch.N
            ws_bytes = L.trajsde_aggregator_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), K)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            legacy = torch.empty(K, N, D, device=dev, dtype=torch.float32)
            _lib.check(L.trajsde_aggregator_forward(C.byref(gc.batch), C.byref(gc.graph), rt.blob().data_ptr(), nl, K, local.data_ptr(),
                                                    ws.data_ptr(), ws_bytes, legacy.data_ptr(), st), "trajsde_aggregator_forward")
            d_glob = gm_inputs["d_glob"]
            grads = rt._grad_buffers(_lib.STAGE_AGGREGATOR_BWD)                          # pre-zeroed, as the header says
            arr, _keep = grads.pointer_array()
            d_local = torch.empty(N, D, device=dev, dtype=torch.float32)
            bws_bytes = L.trajsde_aggregator_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), nl, K)
            bws = torch.empty(bws_bytes, device=dev, dtype=torch.uint8)
            _lib.check(L.trajsde_aggregator_backward(C.byref(gc.batch), C.byref(gc.graph), rt.blob().data_ptr(),
                                                     rt.blob(_lib.STAGE_AGGREGATOR_BWD).data_ptr(), nl, K, local.data_ptr(), d_glob.data_ptr(),
                                                     bws.data_ptr(), bws_bytes, arr, len(grads), d_local.data_ptr(), st),
                       "trajsde_aggregator_backward")
            torch.cuda.synchronize()
            assert torch.equal(plain, prepared) and torch.equal(plain, legacy)
        # (the backward of this asymmetric list scatters with atomics: its outputs are checked for (a) and (b), not compared)
        assert bool(torch.isfinite(d_local).all()) and bool(torch.isfinite(grads.flat).all())
        return {"plain": plain, "prepared": prepared, "legacy": legacy}, [plain, prepared, legacy, d_local, grads.flat, ws, bws, prep.ws]

    gm_inputs = {}

    def make(gm, fill):
        N = on_dev["x"].shape[0]
        gm_inputs["d_glob"] = gm.placed(torch.randn(K, N, D, generator=torch.Generator().manual_seed(4)).to(dev), fill, label="d_global")
        return place_batch(gm, on_dev, fill)
    call.after = lambda gm, data: assert_graph_pointers(gm, data)
    contract("aggregator: prepared, legacy forward and backward", make, call)


def test_encoder_backward_with_the_tape_in_one_buffer(dev):
    """trajsde_encoder_backward with `ws` = tape + scratch in ONE buffer of trajsde_encoder_backward_ws_bytes (scratch = null) and the
    forward recomputed inside, next to the runtime's form (tape from trajsde_encoder_forward_train, separate scratch)"""
    from trajsde_amd import _lib
    from trajsde_amd.runtime import D, GraphContext, NoiseSpec, rotate_inputs
    RAN.add("encoder_backward")
    K, T = 6, 12
    model = sde_model(K, T, dropout=0.0).to(dev)
    rt = model.encoder._rt
    on_dev = _case_batch("nt61_k10_t12").to(dev)
    L = _lib.lib()
    held = {}

    def make(gm, fill):
        held["d_local"] = gm.placed(torch.randn(on_dev["x"].shape[0], D, generator=torch.Generator().manual_seed(5)).to(dev), fill, label="d_local")
        return place_batch(gm, on_dev, fill)

    def call(data):
        noise = NoiseSpec(seed=SEED)
        with torch.no_grad():
            data["rotate_mat"], _ = rotate_inputs(data)
            outs, tape = rt.encoder_forward_train(data, noise)
            two = rt.encoder_backward(data, held["d_local"], noise, diff_weight=0.5, want_boundaries=True, tape=tape)
            gc = GraphContext.get(data, float(model.encoder.local_radius), int(model.encoder.historical_steps), noise)
            tab = rt._enc_table()
            tab_dev = torch.from_numpy(tab).to(dev)
            grads = rt._grad_buffers(_lib.STAGE_ENCODER_BWD)
            arr, _keep = grads.pointer_array()
            loss = torch.empty(1, device=dev, dtype=torch.float32)
            ws_bytes = L.trajsde_encoder_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph))
            assert ws_bytes >= L.trajsde_encoder_tape_bytes(C.byref(gc.batch), C.byref(gc.graph))
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            cn = noise.c_noise(None, None)
            _lib.check(L.trajsde_encoder_backward(
                C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), rt.blob().data_ptr(), rt.blob(_lib.STAGE_ENCODER_BWD).data_ptr(),
                tab.ctypes.data_as(C.c_void_p), tab_dev.data_ptr(), C.byref(cn), held["d_local"].data_ptr(), 0.5, ws.data_ptr(), ws_bytes,
                loss.data_ptr(), arr, len(grads), None, None, None, 0, None, 0, torch.cuda.current_stream().cuda_stream),
                "trajsde_encoder_backward")
            torch.cuda.synchronize()
        return ({"local": outs[0], "grads": grads.flat, "diff_loss": loss, "grads_tape": two["grads"].flat, "diff_loss_tape": two["diff_loss"].reshape(1),
                 "d_latent": two["d_latent"], "d_aa_out": two["d_aa_out"]},
                [outs[0], grads.flat, loss, ws, tape[0], two["grads"].flat, two["d_latent"], two["d_aa_out"]])
    call.after = lambda gm, data: assert_graph_pointers(gm, data)
    contract("encoder backward: one buffer against tape + scratch", make, call)


# ----------------------------------------------------------------------------------------------------------------- the vanilla variant
@pytest.mark.parametrize("name,nll", [("nt63_k6_t30", False), ("n65_k1_t60", True), ("isolated", False)])
def test_vanilla_variant_forward_and_training(name, nll, dev):
    """trajsde_encoder_grid_forward_train / _grid_backward_train, trajsde_aggregator_forward_heads and _backward_heads at 4 heads,
    trajsde_mlp_decoder_forward and both MLP decoder backwards through the vanilla model; then trajsde_encoder_grid_forward and
    trajsde_encoder_grid_backward (the forms without dropout) through ctypes next to the train forms in eval mode"""
    from trajsde_amd import _lib
    from trajsde_amd.runtime import D, GraphContext, rotate_inputs
    RAN.add("vanilla")
    if name in SHAPE_CASES:
        K, T, batch = SHAPE_CASES[name][2], SHAPE_CASES[name][3], _case_batch(name)
    else:
        K, T, batch = 6, 12, degenerate_batch(name, 12)
    model = grid_model(K, T, nll=nll).to(dev)
    forward_contract(f"vanilla forward {name}", model, batch, dev, K, keys=("loc", "pi", "local_embed", "global_embed"), fake_agents=False)
    training_contract(f"vanilla training[{'nll' if nll else 'l2'}] {name}", model, batch, dev, K, compare=name not in ASYMMETRIC)
    rt, L, on_dev, held = model.encoder._rt, _lib.lib(), batch.to(dev), {}
    heads, nl = int(model.encoder.num_heads), int(model.encoder.num_temporal_layers)

    def make(gm, fill):
        held["d_local"] = gm.placed(torch.randn(on_dev["x"].shape[0], D, generator=torch.Generator().manual_seed(5)).to(dev), fill, label="d_local")
        return place_batch(gm, on_dev, fill)

    def call(data):
        st = torch.cuda.current_stream().cuda_stream
        with torch.no_grad():
            data["rotate_mat"], _ = rotate_inputs(data)
            want = rt.encoder_grid_forward(data)
            want_g = rt.encoder_grid_backward(data, held["d_local"])["grads"]
            gc = GraphContext.get(data, None, 21, None)
            N = gc.batch.N
            local = torch.empty(N, D, device=dev, dtype=torch.float32)
            ws_bytes = L.trajsde_encoder_grid_ws_bytes(C.byref(gc.batch), C.byref(gc.graph))
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            _lib.check(L.trajsde_encoder_grid_forward(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), rt.blob().data_ptr(), heads, nl,
                                                      ws.data_ptr(), ws_bytes, local.data_ptr(), st), "trajsde_encoder_grid_forward")
            grads = rt._grad_buffers(_lib.STAGE_ENCODER_GRID_BWD)
            arr, _keep = grads.pointer_array()
            bws_bytes = L.trajsde_encoder_grid_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), nl)
            bws = torch.empty(bws_bytes, device=dev, dtype=torch.uint8)
            _lib.check(L.trajsde_encoder_grid_backward(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), rt.blob().data_ptr(),
                                                       rt.blob(_lib.STAGE_ENCODER_GRID_BWD).data_ptr(), heads, nl, held["d_local"].data_ptr(),
                                                       bws.data_ptr(), bws_bytes, arr, len(grads), st), "trajsde_encoder_grid_backward")
            torch.cuda.synchronize()
        assert torch.equal(local, want)                     # "null or p = 0: identical to trajsde_encoder_grid_forward" (the header)
        return {"local": local, "grads": grads.flat, "grads_train_form": want_g.flat}, [local, grads.flat, ws, bws, want, want_g.flat]
    call.after = lambda gm, data: assert_graph_pointers(gm, data, fake_agents=False)
    contract(f"vanilla encoder without dropout {name}", make, call)


# ----------------------------------------------------------------------------------------------------------------- small launches
def test_pack_weights_for_every_stage(dev):
    """trajsde_pack_weights for every trajsde_stage value and trajsde_pack_weights_many over all of them, parameters placed: the images
    are bit-identical whatever the blobs held before"""
    from trajsde_amd import _lib, runtime
    RAN.add("pack")
    sde, grid = sde_model(6, 12).to(dev), grid_model(6, 12).to(dev)
    stages = [(sde.encoder._rt, (_lib.STAGE_ENCODER, _lib.STAGE_ENCODER_BWD)), (sde.aggregator._rt, (_lib.STAGE_AGGREGATOR, _lib.STAGE_AGGREGATOR_BWD)),
              (sde.decoder._rt, (_lib.STAGE_DECODER, _lib.STAGE_DECODER_BWD, _lib.STAGE_DECODER_NLL_BWD, _lib.STAGE_DECODER_MILSTEIN,
                                 _lib.STAGE_DECODER_MILSTEIN_BWD, _lib.STAGE_DECODER_MILSTEIN_NLL_BWD)),
              (grid.encoder._rt, (_lib.STAGE_ENCODER_GRID, _lib.STAGE_ENCODER_GRID_BWD)),
              (grid.decoder._rt, (_lib.STAGE_DECODER_MLP, _lib.STAGE_DECODER_MLP_BWD, _lib.STAGE_DECODER_MLP_NLL_BWD))]
    entries = [(rt, sid) for rt, sids in stages for sid in sids]
    assert sorted(sid for _, sid in entries) == list(range(15))                            # every value of the enum

    def make(gm, fill):
        for model in (sde, grid):                                                          # every parameter in an arena of its own
            with torch.no_grad():
                for p in model.parameters():
                    p.data = gm.placed(p.data, fill, label="parameter")
            for m in model.modules():
                if hasattr(m, "touch"):
                    m.touch()
                rt = getattr(m, "_rt", None)
                if isinstance(rt, runtime.StageRuntime):
                    rt._blobs.clear()
                    rt.__dict__.pop("_ptr_tables", None)
        return None

    def call(_):
        one = [rt.blob(sid) for rt, sid in entries]
        single = {f"single.{sid}": b.clone() for (_, sid), b in zip(entries, one)}
        for rt, _ in entries:
            rt._blobs.clear()
        ps = runtime.PackSet(entries)
        ps.refresh()
        torch.cuda.synchronize()
        for (_, sid), a, b in zip(entries, one, ps._blobs):
            assert torch.equal(a, b), sid
        return {**single, **{f"many.{sid}": b for (_, sid), b in zip(entries, ps._blobs)}}, one + list(ps._blobs) + [ps._tables[1]]
    contract("pack_weights, every stage", make, call)


def test_sde_step_rows(dev):
    """trajsde_sde_step at row counts around the tile sizes, state and injected noise placed"""
    RAN.add("sde_step")
    sde_step_contract(sde_model(6, 12).to(dev), dev, False)


def sde_step_contract(model, dev, bf16):
    from trajsde_amd import _lib
    from trajsde_amd.schedule import decoder_schedule
    tab = np.ascontiguousarray(decoder_schedule(12, 1.2).step_table())
    e = tab[2].ctypes.data_as(C.POINTER(C.c_float))
    for rows in (1, 15, 16, 17, 63, 64, 65, 117):
        g = torch.Generator().manual_seed(rows)
        y, z = torch.randn(rows, 64, generator=g).to(dev), torch.randn(1, rows, 64, generator=g).to(dev)
        if bf16:
            y = y.to(torch.bfloat16)
        held = {}

        def make(gm, fill):
            held["y"], held["z"] = gm.placed(y, fill, label="y_in"), gm.placed(z, fill, label="z")
            return None

        def call(_):
            out = torch.empty_like(held["y"])
            out2 = torch.empty_like(held["y"])
            st = torch.cuda.current_stream().cuda_stream
            nz = _lib.Noise(C.c_uint64(0), held["z"].data_ptr(), None, None)
            _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), held["y"].data_ptr(), out.data_ptr(), e, 0,
                                                   C.byref(nz), st), "trajsde_sde_step")          # (z holds one step: step index 0)
            nz2 = _lib.Noise(C.c_uint64(3), None, None, None)                              # in-kernel Philox
            _lib.check(_lib.lib().trajsde_sde_step(rows, model.decoder._rt.blob().data_ptr(), held["y"].data_ptr(), out2.data_ptr(), e, 2,
                                                   C.byref(nz2), st), "trajsde_sde_step")
            return {"injected": out.float(), "philox": out2.float()}, [out, out2]
        contract(f"sde_step rows={rows} bf16={bf16}", make, call)


def test_gather_add_and_adamw_launches(dev):
    """trajsde_grad_gather_add (three items, with and without the device scalar) and trajsde_adamw_step at 1, 7, 1000 and 530 001
    elements (tests/test_gpu_step_launches.py), every operand in an arena"""
    from trajsde_amd import _lib
    RAN.add("step_launches")
    L = _lib.lib()
    g = torch.Generator().manual_seed(1)
    flat0, scale0 = torch.randn(5000, generator=g), torch.tensor([0.37])
    srcs0 = [torch.randn(k, generator=g) for k in (900, 2500, 64)]
    idx0 = [torch.randperm(s.numel(), generator=g)[:k] for s, k in zip(srcs0, (700, 2500, 1))]
    firsts, mults = (10, 1000, 4999), (1.0, 0.25, 3.0)
    held = {}

    def make(gm, fill):
        held["flat"] = gm.placed(flat0.to(dev), fill, label="flat", const=False)
        held["scale"] = gm.placed(scale0.to(dev), fill, label="scale")
        held["srcs"] = [gm.placed(s.to(dev), fill, label="src") for s in srcs0]
        held["idx"] = [gm.placed(i.to(dev), fill, label="index") for i in idx0]            # guards 0 / 1: valid positions of every src
        return None

    def call(_):
        items = (_lib.GatherItem * 3)()
        for it, f, s, i, m in zip(items, firsts, held["srcs"], held["idx"], mults):
            it.dst, it.src, it.index, it.n, it.mult = held["flat"].data_ptr() + 4 * f, s.data_ptr(), i.data_ptr(), i.numel(), m
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.trajsde_grad_gather_add(items, 3, held["scale"].data_ptr(), st), "trajsde_grad_gather_add")
        _lib.check(L.trajsde_grad_gather_add(items, 3, None, st), "trajsde_grad_gather_add")
        torch.empty(1, device=dev)                                                          # (the context routed something)
        return {"flat": held["flat"]}, []
    contract("grad_gather_add", make, call)

    for n in (1, 7, 1000, 530_001):
        gn = torch.Generator().manual_seed(n)
        p0, g0, m0, v0 = (torch.randn(n, generator=gn) for _ in range(4))

        def make_a(gm, fill):
            held["p"], held["m"], held["v"] = (gm.placed(t.to(dev), fill, label=k, const=False) for t, k in ((p0, "param"), (m0, "exp_avg"), (v0.abs(), "exp_avg_sq")))
            held["g"] = gm.placed(g0.to(dev), fill, label="grad")
            return None

        def call_a(_):
            lr, wd, b1, b2, step = 3e-3, 1e-2, 0.9, 0.999, 3
            for divide, bias2 in ((1, (1 - b2 ** step) ** 0.5), (0, 1.0 / (1 - b2 ** step) ** 0.5)):
                _lib.check(L.trajsde_adamw_step(held["p"].data_ptr(), held["g"].data_ptr(), held["m"].data_ptr(), held["v"].data_ptr(), n,
                                                1 - lr * wd, 1 - b1, b2, 1 - b2, bias2, divide, 1e-8, -(lr / (1 - b1 ** step)),
                                                torch.cuda.current_stream().cuda_stream), "trajsde_adamw_step")
            torch.empty(1, device=dev)
            return {"param": held["p"], "exp_avg": held["m"], "exp_avg_sq": held["v"]}, []
        contract(f"adamw_step n={n}", make_a, call_a)


# ----------------------------------------------------------------------------------------------------------------- other kernel forms
_CHILD = os.path.join(H.ROOT, "tests", "memory_contract_child.py")


def _run_child(args, env):
    r = subprocess.run([sys.executable, _CHILD] + list(args), env={**os.environ, **env}, timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, f"child {args} {env} failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ok"] and verdict["runs"] > 0, verdict
    return verdict


def test_every_kernel_form_keeps_the_contract(dev):
    """the switch matrix of test_gpu_trained_weights: one child interpreter per form, one after the other, each with one mixed and
    one degenerate batch, forward and training step"""
    import test_gpu_trained_weights as W
    for mode, env in W._MODES:
        v = _run_child(["forms"], env)
        print(f"[memory-contract] kernel form {mode}: {v}")


def test_strict24_library_keeps_the_contract(dev):
    """the bf16x6 twin (variants/libtrajsde_strict24.so, made by build()), the same child: its larger edge image makes
    edge_embed_backward (csrc/node_bwd.hip) run its attention form with four store tiles in LDS instead of eight"""
    from trajsde_amd import build
    if not os.path.isfile(build.STRICT_LIB):
        pytest.skip("variants/libtrajsde_strict24.so not built")
    print("[memory-contract] strict24:", _run_child(["forms"], {"TRAJSDE_LIB": build.STRICT_LIB}))


def test_bf16_state_storage_keeps_the_contract(dev):
    """trajsde_state_storage(1) (bf16 rows inside the stages; process-wide, so a child of its own): the inference forward and
    trajsde_sde_step on bf16 states"""
    print("[memory-contract] bf16 state storage:", _run_child(["bf16"], {}))


def test_full_size_step_does_not_depend_on_what_memory_held(dev):
    """one training step of BASELINE config2 (grids wrap, partial sums are deferred) in four fresh processes whose allocator was
    pre-filled with nothing, NaN, zeros and random bits (tests/grad_digest_child.py, TRAJSDE_TEST_POISON): the four JSON lines -- loss
    and the digests of all gradients -- are equal, and every gradient is finite"""
    lines = []
    for poison in (None, "nan", "zero", "7"):
        env = {k: v for k, v in os.environ.items() if k != "TRAJSDE_TEST_POISON"}
        if poison is not None:
            env["TRAJSDE_TEST_POISON"] = poison
        r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "grad_digest_child.py"), "config2"], env=env, timeout=900,
                           capture_output=True, text=True)
        assert r.returncode == 0, f"poison {poison}: child failed ({r.returncode}):\n{r.stderr[-6000:]}"
        lines.append(r.stdout.strip().splitlines()[-1])
        got = json.loads(lines[-1])
        assert np.isfinite(got["loss"]) and len(got["digests"]) > 100 and all(d[2] for d in got["digests"].values()), poison
        print(f"[memory-contract] config2 step, poison {poison}: loss {got['loss']!r}")
    assert lines[1] == lines[0] and lines[2] == lines[0] and lines[3] == lines[0]


# ----------------------------------------------------------------------------------------------------------------- accounting
# every symbol of _lib.SIGNATURES that launches work or writes device memory -> the RAN tags of the tests that call it
LAUNCHES = {
    "trajsde_rotate": ("forward",), "trajsde_graph_prepare": ("training", "capture"), "trajsde_graph_prepare_async": ("forward",),
    "trajsde_graph_compact": ("forward",), "trajsde_encoder_forward": ("forward", "capture"), "trajsde_encoder_forward_ood": ("capture",),
    "trajsde_encoder_forward_train": ("training",), "trajsde_encoder_backward": ("training", "encoder_backward"),
    "trajsde_aggregator_forward": ("aggregator",), "trajsde_aggregator_forward_heads": ("forward", "vanilla"),
    "trajsde_aggregator_prepare": ("aggregator",), "trajsde_aggregator_forward_prepared": ("aggregator",),
    "trajsde_aggregator_forward_train": ("training",), "trajsde_aggregator_backward": ("aggregator",),
    "trajsde_aggregator_backward_heads": ("training", "vanilla"), "trajsde_decoder_forward": ("forward",),
    "trajsde_decoder_forward_milstein": ("forward",), "trajsde_decoder_l2_backward": ("training",), "trajsde_decoder_nll_backward": ("training",),
    "trajsde_decoder_l2_backward_milstein": ("training",), "trajsde_decoder_nll_backward_milstein": ("training",),
    "trajsde_sde_step": ("sde_step",), "trajsde_encoder_grid_forward": ("vanilla",), "trajsde_encoder_grid_forward_train": ("vanilla",),
    "trajsde_encoder_grid_backward": ("vanilla",), "trajsde_encoder_grid_backward_train": ("vanilla",),
    "trajsde_mlp_decoder_forward": ("vanilla",), "trajsde_mlp_decoder_l2_backward": ("vanilla",), "trajsde_mlp_decoder_nll_backward": ("vanilla",),
    "trajsde_pack_weights": ("pack",), "trajsde_pack_weights_many": ("pack", "training"), "trajsde_grad_gather_add": ("step_launches",),
    "trajsde_adamw_step": ("step_launches",),
}
# ... and the ones left out, each with its reason
NOT_EXERCISED = {
    "trajsde_range_status": "reads (and clears) the library's own sticky word, takes no caller buffer on the device; sites_out is a host pointer",
    "trajsde_encoder_fork_stream": "records an event and makes a stream wait; no memory is touched",
    "trajsde_profile_mode": "host-side switch of the event recorder",
    "trajsde_profile_report": "formats the recorder's timings into a HOST buffer of the given capacity",
}
QUERIES = {"trajsde_last_error", "trajsde_split_products", "trajsde_abi_version", "trajsde_export_senders", "trajsde_state_storage",
           "trajsde_param_count", "trajsde_param_name", "trajsde_blob_floats", "trajsde_pack_many_table_bytes", "trajsde_sync_free_supported",
           "trajsde_radius2_threshold"}                         # host-only: they return a number or a string (with every *_bytes query)


def test_zz_every_launch_entry_point_is_accounted_for(dev):
    """every symbol of _lib.SIGNATURES is a size / host query, or listed in LAUNCHES, or excluded with a reason; and each launch entry
    point was really called (the spy of `dev`) by the tests of this module that claim it, when they ran"""
    from trajsde_amd import _lib
    names = set(_lib.SIGNATURES)
    queries = QUERIES | {n for n in names if n.endswith("_bytes")}
    assert not (set(LAUNCHES) | set(NOT_EXERCISED) | QUERIES) - names, "the tables name symbols the binding does not have"
    assert not set(LAUNCHES) & set(NOT_EXERCISED) and not set(LAUNCHES) & queries
    unaccounted = names - queries - set(LAUNCHES) - set(NOT_EXERCISED)
    assert not unaccounted, f"entry points without a memory-contract test: {sorted(unaccounted)}"
    assert len(NOT_EXERCISED) <= 4 and all(len(r) > 20 for r in NOT_EXERCISED.values())
    missed = sorted(n for n, tags in LAUNCHES.items() if all(t in RAN for t in tags) and n not in CALLED)
    print(f"[memory-contract] {len(LAUNCHES)} launch entry points, {len(CALLED & set(LAUNCHES))} called in this run, tests run: {sorted(RAN)}")
    assert not missed, f"listed as exercised but never called: {missed}"


QUANTITIES = ("N", "Nt", "K*N", "H*Nt", "E", "E_aa", "E_g", "E_la")


def test_zz_row_counts_reach_every_residue_class(dev):
    """the row counts the cases above really had (printed): each of N, Nt, K*N, H*Nt, E, E_aa, E_g and E_la was 1 below, equal to and
    1 above a multiple of 16 and of 64"""
    if not {"forward", "training"} <= RAN:
        pytest.skip("needs the shape cases of this module to have run in the same session")
    rows = [r for r in COUNTS if r["case"].split()[-1] in SHAPE_CASES]
    for r in rows:
        print("[memory-contract]", r)
    missing = []
    for q in QUANTITIES:
        for mod in (16, 64):
            for res in (mod - 1, 0, 1):
                if not any(r[q] > 0 and r[q] % mod == res for r in rows):
                    missing.append((q, mod, res))
    assert not missing, missing
