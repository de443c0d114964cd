"""Cross-stream handoffs with the producing or the reading stream held back (-m gpu).

The runtime orders work across streams with events (`StageRuntime.blob`, `prefetch_graph`, `RelPrefetch.join`, the loader's
`_hand_over`), with `wait_stream` (`PackSet.refresh`) and with `record_stream` (blocks made on one stream and used on another).  At test
shapes the producing stream has drained before the consumer's first kernel starts, so none of that ordering can fail a test by itself.
Here the stream that matters is kept busy by `stream_tools.hold` while the other stream's work is enqueued (`assert_still_held`: the
precondition of every such test, never skipped), and blocks that may not be reused yet are asked for again and filled with NaNs
(`stream_tools.poison`).  Expected values are serial: the same call on the default stream with a device synchronisation before and
after, compared bit for bit -- every inference launch is bit-reproducible; the serial outputs of one batch are held to the oracle once.
Findings are printed as "[streams] ..." lines: per held test the hold's measured length against the host time of the enqueue."""
import os

import pytest
import torch

import helpers as H
import stream_tools as ST

pytestmark = pytest.mark.gpu

K, T, MAX_T = 3, 6, 0.5
T_TRAIN, MAX_T_TRAIN = 20, 2.0
SHAPES = ((2, 9, 6), (4, 40, 12), (3, 17, 6), (1, 65, 8))        # (S, n, L): workspaces differ, 65 crosses a 64-row tile
KEYS = ("loc", "pi", "diff_in", "diff_out")
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    d = torch.device("cuda:0")
    ST._calibrate(d)
    return d


@pytest.fixture(scope="module")
def streams(dev):
    """the three streams of this module's own (the library's side streams come on top)"""
    return [torch.cuda.Stream(device=dev) for _ in range(3)]


def host_batches(F):
    from trajsde_amd.synth import synth
    return [synth(S=S, n=n, L=L, F=F, box=60.0, seed=70 + i, mixed_source=True, history_dropout=0.2) for i, (S, n, L) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def small(dev):
    return host_batches(T)


@pytest.fixture(scope="module")
def small_train(dev):
    return host_batches(T_TRAIN)


def on_device(batch, dev):
    """a fresh device copy made on the default stream and complete before anything else is enqueued"""
    b = H.clone_batch(batch).to(dev)
    torch.cuda.synchronize()
    return b


def pinned(batch):
    from trajsde_amd.data import TemporalData
    return TemporalData(**{k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in H.clone_batch(batch).as_dict().items()})


def keep(out, keys=KEYS):
    """the outputs a test compares, cloned on the current stream"""
    return {k: out[k].clone() for k in keys if k in out}


def serial(call, keys=KEYS):
    """the expected value: `call()` alone on the default stream, the device idle before and after"""
    torch.cuda.synchronize()
    with torch.no_grad():
        out = keep(call(), keys)
    torch.cuda.synchronize()
    return out


def same(got, want, tag, finite=True):
    assert got.keys() == want.keys() and len(want) >= 2, (tag, sorted(got), sorted(want))
    for k in want:
        if finite and want[k].is_floating_point():
            assert bool(torch.isfinite(want[k]).all()), (tag, k, "the serial value itself is not finite")
        assert torch.equal(got[k], want[k]), (tag, k, H.maxdiff(got[k].float().cpu(), want[k].float().cpu()))


def spec(seed):
    from trajsde_amd.runtime import NoiseSpec
    return NoiseSpec(seed=seed)


def sde_model(dev, T_=T, max_t=MAX_T, init_seed=7, method="euler"):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, T_, max_t)
    if method == "milstein":
        cfg["decoder"]["kwargs"]["method"] = cfg["encoder"]["kwargs"]["method"] = "milstein"
    return PredictionModelSDENet(**cfg, init_seed=init_seed).eval().to(dev), cfg


def stage_rts(model):
    return [model.encoder._rt, model.aggregator._rt, model.decoder._rt]


def edit_weights(model, delta=0.25):
    """add `delta` in place to one bias of every stage (on the current stream): the version counters move, the next blob() or
    PackSet.refresh() re-packs"""
    with torch.no_grad():
        for stage in (model.encoder, model.aggregator, model.decoder):
            name = next(n for n in stage._rt.param_names() if n.endswith(".bias"))
            stage.p(name).add_(delta)


# ------------------------------------------------------------------------------------------------------------ the serial reference itself
@pytest.fixture(scope="module")
def main_model(dev):
    return sde_model(dev)


def test_serial_outputs_are_the_oracles(dev, small, main_model):
    """what every test below compares with -- the forward alone on the default stream -- against the oracle at the suite's 1e-4"""
    model, cfg = main_model
    b = small[2]
    got = serial(lambda: model(on_device(b, dev), noise=spec(102)))
    want = H.oracle_forward(model, cfg, b, noise_seed=102, want_intermediates=False)
    for k in ("loc", "pi"):
        err = H.maxdiff(got[k].cpu(), want[k])
        print(f"[streams] serial forward against the oracle: {k} {err:.2e}")
        assert err <= TOL, (k, err)


# ------------------------------------------------------------------------------------------------------------ 1. interleaved forwards
def _variant(name, dev):
    """(model, call(model, batch, seed) -> outputs, compared keys, _OVERLAP_REL during the interleaved run)"""
    plain = lambda m, b, s: m(b, noise=spec(s))                         # noqa: E731
    if name == "sde":
        return sde_model(dev)[0], plain, KEYS, False
    if name == "overlap_rel":
        return sde_model(dev)[0], plain, KEYS, True
    if name == "milstein":
        return sde_model(dev, method="milstein")[0], plain, KEYS, False
    if name == "mc":
        return sde_model(dev)[0], (lambda m, b, s: m.predict_samples(b, 5, noise=spec(s))), KEYS + ("loc_mean", "loc_cov"), False
    from trajsde_amd.models.model_base_mix import PredictionModel
    return PredictionModel(**H.grid_cfg(K, T, 4, 2, dropout=0.0), init_seed=9).eval().to(dev), plain, ("loc", "pi"), False


@pytest.mark.parametrize("variant", ["sde", "overlap_rel", "milstein", "mc", "vanilla"])
def test_interleaved_forwards_are_the_serial_forwards(variant, dev, small, streams):
    """12 forwards dealt over three streams (step i on stream i % 3, batch i % 4, seed 100 + i) without a synchronisation in between:
    bit for bit the 12 serial forwards.  The relative-pose prefetch variant is compared with the serial forwards of the DEFAULT route."""
    from trajsde_amd import runtime
    model, call, keys, overlap = _variant(variant, dev)
    want = [serial(lambda: call(model, on_device(small[i % 4], dev), 100 + i), keys) for i in range(12)]
    staged = [on_device(small[i % 4], dev) for i in range(12)]
    prev = runtime._OVERLAP_REL
    runtime._OVERLAP_REL = overlap
    got = []
    try:
        torch.cuda.synchronize()
        with torch.no_grad():
            for i in range(12):
                with torch.cuda.stream(streams[i % 3]):
                    got.append(keep(call(model, staged[i], 100 + i), keys))
        torch.cuda.synchronize()
    finally:
        runtime._OVERLAP_REL = prev
    for i in range(12):
        same(got[i], want[i], (variant, i))


# ------------------------------------------------------------------------------------------------------------ 2. cold image, held packer
def test_cold_image_packed_on_a_held_stream(dev, small, streams):
    """a fresh model's first forward runs on stream A behind a hold -- its packs are queued, not done -- and at once another batch's
    forward runs on B, which reads the same images: blob() must make B wait for the pack-done event, or B reads torch.empty memory.
    The decoder's schedule tables of this `max_fut_t` (0.7, no other test's) are made by the serial run first: a cold table is uploaded
    by a blocking copy on the current stream, i.e. the host itself would wait for the held stream and nothing could overtake it."""
    A, B = streams[0], streams[1]
    ref, _ = sde_model(dev, max_t=0.7, init_seed=21)
    want_a = serial(lambda: ref(on_device(small[0], dev), noise=spec(1)))
    want_b = serial(lambda: ref(on_device(small[3], dev), noise=spec(2)))
    fresh, _ = sde_model(dev, max_t=0.7, init_seed=21)
    assert all(not rt._blobs for rt in stage_rts(fresh))
    ba, bb = on_device(small[0], dev), on_device(small[3], dev)
    ev = ST.hold(A)
    with torch.no_grad():
        with torch.cuda.stream(A):
            got_a = keep(fresh(ba, noise=spec(1)))
        with torch.cuda.stream(B):
            got_b = keep(fresh(bb, noise=spec(2)))
    ST.assert_still_held(ev, "cold image: forward on B enqueued while A's packs wait behind the hold")
    torch.cuda.synchronize()
    ST.report(ev, "cold image packed on a held stream")
    for rt in stage_rts(fresh):
        assert rt._blobs[rt.stage_id][3] == A.cuda_stream and B.cuda_stream in rt._readers[rt.stage_id]
    same(got_a, want_a, "packer's own forward")
    same(got_b, want_b, "reader on the other stream")


# ------------------------------------------------------------------------------------------------------------ 3. in-place re-pack
def _stage_entries(model):
    from test_gpu_step_launches import _stage_entries as entries
    return entries(model)


def test_in_place_repack_waits_for_a_held_reader(dev, small, streams):
    """PackSet.refresh() zeroes and re-packs the images where they are: a forward with the OLD weights queued on B behind a hold must be
    through before the pack on A starts (`packing.wait_stream(reader)`), the forward on A behind the pack sees the new weights, and so
    does B's next forward (pack-done event)"""
    from trajsde_amd import runtime
    A, B = streams[0], streams[1]
    model, _ = sde_model(dev, init_seed=23)
    twin, _ = sde_model(dev, init_seed=23)
    want_old = serial(lambda: twin(on_device(small[1], dev), noise=spec(5)))
    edit_weights(twin)
    want_new_a = serial(lambda: twin(on_device(small[3], dev), noise=spec(6)))
    want_new_b = serial(lambda: twin(on_device(small[1], dev), noise=spec(7)))
    assert not torch.equal(want_old["loc"], want_new_b["loc"])
    ps = runtime.PackSet(_stage_entries(model))
    ps.refresh()                                                          # (the table's first upload waits on the host: warm before the hold)
    with torch.no_grad():
        model(on_device(small[1], dev), noise=spec(5))
    b1, b2, b3 = on_device(small[1], dev), on_device(small[3], dev), on_device(small[1], dev)
    ptrs = [b.data_ptr() for b in ps._blobs]
    ev = ST.hold(B)
    with torch.no_grad():
        with torch.cuda.stream(B):
            got_old = keep(model(b1, noise=spec(5)))
        with torch.cuda.stream(A):
            edit_weights(model)
            ps.refresh()
            got_new_a = keep(model(b2, noise=spec(6)))
        ST.assert_still_held(ev, "in-place re-pack: edit, refresh and forward on A enqueued while B's reader waits behind the hold")
        with torch.cuda.stream(B):
            got_new_b = keep(model(b3, noise=spec(7)))
    torch.cuda.synchronize()
    ST.report(ev, "in-place re-pack behind a held reader")
    assert [b.data_ptr() for b in ps._blobs] == ptrs                     # re-packed where they were
    same(got_old, want_old, "reader of the old images")
    same(got_new_a, want_new_a, "forward behind the re-pack")
    same(got_new_b, want_new_b, "the old reader's next forward")


def _train_model(dev, init_seed=25):
    from trajsde_amd import driver
    model, _ = sde_model(dev, T_=T_TRAIN, max_t=MAX_T_TRAIN, init_seed=init_seed)
    model.lr, model.weight_decay, model.T_max = 1e-2, 1e-4, 4
    flat = driver.FlatTraining(model)
    return model, flat


def _step(model, flat, batch, seed):
    from trajsde_amd.runtime import NoiseSpec
    model.train()
    flat.zero()
    loss = model.training_step(batch, 0, noise=NoiseSpec(seed=seed, dropout_seed=seed + 1))
    loss.backward()
    flat.step()
    return loss.detach()


def test_training_step_repack_waits_for_a_held_reader(dev, small_train, streams):
    """the same through the training loop's own PackSet: an eval-mode forward on B (a validation stream) is queued behind a hold, then
    one training step + optimizer step and the step's re-pack run on A; B keeps the weights it started with, A and B's next forward
    see the updated ones.  Expected values: a twin that takes the same two steps with the device idle around every call."""
    A, B = streams[0], streams[1]
    model, flat = _train_model(dev)
    twin, tflat = _train_model(dev)
    for m, f in ((twin, tflat), (model, flat)):                          # one step first: the set exists, its tables are uploaded
        _step(m, f, on_device(small_train[0], dev), 40)
        m._step_pack_set().refresh()
        torch.cuda.synchronize()
    twin.eval()
    want_old = serial(lambda: twin(on_device(small_train[2], dev), noise=spec(8)))
    want_loss = _step(twin, tflat, on_device(small_train[1], dev), 42).clone()
    twin._step_pack_set().refresh()
    twin.eval()
    want_new_a = serial(lambda: twin(on_device(small_train[3], dev), noise=spec(9)))
    want_new_b = serial(lambda: twin(on_device(small_train[2], dev), noise=spec(10)))
    assert not torch.equal(want_old["loc"], want_new_b["loc"])
    b1, bt, b2, b3 = (on_device(small_train[i], dev) for i in (2, 1, 3, 2))
    ev = ST.hold(B, 0.5)                                                  # (a whole training step is enqueued under this one)
    model.eval()
    with torch.no_grad(), torch.cuda.stream(B):
        got_old = keep(model(b1, noise=spec(8)))
    with torch.cuda.stream(A):
        loss = _step(model, flat, bt, 42)
        model._step_pack_set().refresh()
        model.eval()
        with torch.no_grad():
            got_new_a = keep(model(b2, noise=spec(9)))
    ST.assert_still_held(ev, "training step re-pack: step, refresh and forward on A enqueued while B's reader waits behind the hold")
    with torch.no_grad(), torch.cuda.stream(B):
        got_new_b = keep(model(b3, noise=spec(10)))
    torch.cuda.synchronize()
    ST.report(ev, "training step's re-pack behind a held reader")
    assert torch.equal(loss, want_loss)
    same(got_old, want_old, "validation forward of the weights before the step")
    same(got_new_a, want_new_a, "forward behind the step's re-pack")
    same(got_new_b, want_new_b, "the validation stream's next forward")


# ------------------------------------------------------------------------------------------------------------ 4. re-pack by replacement
def test_repack_by_replacement_keeps_the_old_image_for_a_held_reader(dev, small, streams):
    """without a PackSet a changed parameter makes blob() allocate a NEW image and drop the old one, whose block goes back to the packing
    stream's pool -- while a forward queued on B behind a hold still reads it through a raw pointer.  Blocks of the old images' sizes are
    asked for again on A at once and filled with NaNs: B must still give the old weights' forward."""
    A, B = streams[0], streams[1]
    model, _ = sde_model(dev, init_seed=27)
    twin, _ = sde_model(dev, init_seed=27)
    want_old = serial(lambda: twin(on_device(small[1], dev), noise=spec(11)))
    with torch.no_grad(), torch.cuda.stream(A):                          # the images are packed on A: their blocks are of A's pool
        model(on_device(small[1], dev), noise=spec(11))
    torch.cuda.synchronize()
    old = [rt._blobs[rt.stage_id][0] for rt in stage_rts(model)]
    old_ptrs, old_bytes = [b.data_ptr() for b in old], [b.numel() * b.element_size() for b in old]
    del old
    b1, b2 = on_device(small[1], dev), on_device(small[3], dev)
    ev = ST.hold(B)
    with torch.no_grad():
        with torch.cuda.stream(B):
            got_old = keep(model(b1, noise=spec(11)))
        with torch.cuda.stream(A):
            edit_weights(model)
            got_new = keep(model(b2, noise=spec(12)))
    bad = ST.poison(A, old_bytes)
    ST.assert_still_held(ev, "re-pack by replacement: new images and poison on A enqueued while B's reader waits behind the hold")
    hit = ST.landed_on(bad, old_ptrs)
    torch.cuda.synchronize()
    ST.report(ev, "re-pack by replacement behind a held reader")
    print(f"[streams] re-pack by replacement: {hit} of {len(old_ptrs)} old images' addresses were handed out again (and filled with NaNs) "
          "while the held reader had not run")
    assert [rt._blobs[rt.stage_id][0].data_ptr() for rt in stage_rts(model)] != old_ptrs
    edit_weights(twin)
    same(got_new, serial(lambda: twin(on_device(small[3], dev), noise=spec(12))), "forward on the new images")
    for k, v in got_old.items():
        assert bool(torch.isfinite(v).all()), (k, "the held reader read a block that had been handed out again")
    same(got_old, want_old, "held reader of the replaced images")


# ------------------------------------------------------------------------------------------------------------ 5. prefetch_graph
def _prefetch_sizes(b, gc):
    from trajsde_amd.runtime import _tensors_in
    ts = [t for t in _tensors_in(list(b.as_dict().values()) + [gc.ws, gc.edges_ws, gc.rot] + list(gc._keep)) if t.is_cuda]
    return sorted({t.data_ptr(): t.numel() * t.element_size() for t in ts if t.numel()}.values())


@pytest.mark.parametrize("drop", [False, True], ids=["kept", "dropped_and_poisoned"])
def test_prefetch_graph_on_a_held_side_stream(drop, dev, small, main_model):
    """the batch is copied, rotated and run through the graph stage on the side stream behind a hold; the eval forward on the main stream
    is enqueued at once and must wait for the event.  `dropped_and_poisoned`: the batch and every reference to it are dropped right after
    the forward was enqueued and blocks of its tensors' sizes are asked for again on the side stream and filled with 0xFF: record_stream
    must have kept them for the main stream's kernels."""
    import weakref
    from trajsde_amd import runtime
    model, _ = main_model
    main, side = torch.cuda.default_stream(dev), runtime.side_stream(dev)
    want = serial(lambda: model(on_device(small[1], dev), noise=spec(13)))
    host = pinned(small[1])
    torch.cuda.synchronize()
    ev = ST.hold(side)
    with torch.cuda.stream(side):
        b = host.to(dev, non_blocking=True)
        model.prefetch_graph(b, spec(13), main_stream=main)
    assert runtime.ROTATED_KEY in b
    with torch.no_grad():
        got = keep(model(b, noise=spec(13)))
    bad = None
    if drop:
        sizes = _prefetch_sizes(b, b[runtime.GraphContext.KEY])
        gone = weakref.ref(b["x"])
        del b
        assert gone() is None                                             # (no cycle keeps the batch: its blocks are back with the allocator)
        bad = ST.poison(side, sizes)
    ST.assert_still_held(ev, "prefetch_graph: forward on the main stream enqueued while the side stream waits behind the hold")
    torch.cuda.synchronize()
    ST.report(ev, f"prefetch_graph on a held side stream ({'dropped and poisoned' if drop else 'kept'})")
    same(got, want, "forward of the prefetched batch")
    del bad


def test_prefetched_training_step_on_a_held_side_stream(dev, small_train):
    """one training step of a batch prefetched behind a hold: loss and gradients bit for bit those of the plain batch.  The step itself
    reads the graph's list lengths on the side stream (GraphContext.make_exact) and so waits for the hold on the host: the precondition
    is taken where the step is entered."""
    from trajsde_amd import runtime
    from trajsde_amd.runtime import NoiseSpec
    model, _ = sde_model(dev, T_=T_TRAIN, max_t=MAX_T_TRAIN, init_seed=29)
    model.train()
    main, side = torch.cuda.default_stream(dev), runtime.side_stream(dev)
    noise = NoiseSpec(seed=33, dropout_seed=34)

    def step(b):
        model.zero_grad(set_to_none=True)
        loss = model.training_step(b, 0, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    want_loss, want = step(on_device(small_train[1], dev))
    host = pinned(small_train[1])
    torch.cuda.synchronize()
    ev = ST.hold(side)
    with torch.cuda.stream(side):
        b = host.to(dev, non_blocking=True)
        model.prefetch_graph(b, noise, main_stream=main)
    ST.assert_still_held(ev, "prefetched training step: the step is entered while the side stream waits behind the hold")
    got_loss, got = step(b)
    ST.report(ev, "prefetched training step on a held side stream")
    assert torch.equal(got_loss, want_loss) and bool(torch.isfinite(got_loss))
    assert got.keys() == want.keys() and len(want) > 100
    for n in want:
        assert torch.equal(got[n], want[n]), n


PLAIN_KEYS = ("x", "y", "rotate_mat", "positions", "padding_mask", "edge_index", "agent_index", "lane_actor_index")


@pytest.mark.parametrize("drop", [False, True], ids=["kept", "dropped_and_poisoned"])
def test_prefetch_graph_hand_off_under_plain_reads(drop, dev, small, main_model):
    """the same hand-off with the plainest consumer there is: the main stream copies the batch's tensors, the rotated `y` and
    `rotate_mat` among them, while the side stream that makes them waits behind the hold; with `dropped_and_poisoned` their blocks are
    asked for again on the side stream as soon as the copies are enqueued.  (A consumer that dereferences nothing: what it reads too
    early, or after the block was handed out again, can only be a wrong value.)"""
    from trajsde_amd import runtime
    model, _ = main_model
    main, side = torch.cuda.default_stream(dev), runtime.side_stream(dev)
    plain = on_device(small[1], dev)
    model._ensure_rotated(plain)
    torch.cuda.synchronize()
    want = {k: plain[k].clone() for k in PLAIN_KEYS}
    host = pinned(small[1])
    torch.cuda.synchronize()
    ev = ST.hold(side)
    with torch.cuda.stream(side):
        b = host.to(dev, non_blocking=True)
        model.prefetch_graph(b, spec(13), main_stream=main)
    got = {k: b[k].clone() for k in PLAIN_KEYS}
    bad = None
    if drop:
        sizes = _prefetch_sizes(b, b[runtime.GraphContext.KEY])
        del b
        bad = ST.poison(side, sizes)
    ST.assert_still_held(ev, "prefetch_graph: copies on the main stream enqueued while the side stream waits behind the hold")
    torch.cuda.synchronize()
    ST.report(ev, f"prefetch_graph under plain reads ({'dropped and poisoned' if drop else 'kept'})")
    for k in PLAIN_KEYS:
        assert torch.equal(got[k], want[k]), k
    del bad


# ------------------------------------------------------------------------------------------------------------ 6. relative-pose prefetch
@pytest.mark.parametrize("where", ["default_stream", "own_stream_beside_another"])
def test_relative_pose_prefetch_with_its_side_stream_held(where, dev, small, streams, main_model):
    """TRAJSDE_OVERLAP_REL: the side stream the relative-pose rows are made on is held before the forward starts, so the aggregator on
    the forward's stream is enqueued long before the rows exist: RelPrefetch.join must make it wait.  Expected: the default route."""
    from trajsde_amd import runtime
    import ctypes as C
    from trajsde_amd import _lib
    model, _ = main_model
    ref = on_device(small[1], dev)
    want = serial(lambda: model(ref, noise=spec(14)))
    want2 = serial(lambda: model(on_device(small[3], dev), noise=spec(15)))
    cur = torch.cuda.default_stream(dev) if where == "default_stream" else streams[0]
    side = runtime._side_stream(dev, cur)
    # the rows' workspace comes from the side stream's pool, where a block of that size may still hold the rows of an earlier forward
    # of this very batch: a block of exactly its size is filled with NaNs and given back first, so rows read too early are not the right ones
    gc = ref[runtime.GraphContext.KEY]
    ws_bytes = int(_lib.lib().trajsde_aggregator_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), K))
    stale = ST.poison(side, [ws_bytes])
    torch.cuda.synchronize()
    del stale
    b1, b2 = on_device(small[1], dev), on_device(small[3], dev)
    prev = runtime._OVERLAP_REL
    runtime._OVERLAP_REL = True
    got2 = None
    try:
        ev = ST.hold(side)
        with torch.no_grad():
            with torch.cuda.stream(cur):
                got = keep(model(b1, noise=spec(14)))
            if where != "default_stream":
                with torch.cuda.stream(streams[1]):
                    got2 = keep(model(b2, noise=spec(15)))
        ST.assert_still_held(ev, "relative-pose prefetch: the forward is enqueued while its side stream waits behind the hold")
        torch.cuda.synchronize()
    finally:
        runtime._OVERLAP_REL = prev
    ST.report(ev, f"relative-pose prefetch, side stream held ({where})")
    same(got, want, "forward whose side stream was held")
    if got2 is not None:
        same(got2, want2, "forward on the other stream")


# ------------------------------------------------------------------------------------------------------------ 7. loader hand-over
class Through:
    """`base` with some attributes replaced: what the loader's module sees as `torch` while its iterator starts"""

    def __init__(self, base, **over):
        self.__dict__.update(_base=base, **over)

    def __getattr__(self, name):
        return getattr(self._base, name)


def _scene_loader(tmp_path, dev):
    """(loader over the tiny scene shards of test_dataset_fed_batches_match_oracle, its one host batch)"""
    import numpy as np
    from test_dataset import BASE, _groups
    from trajsde_amd.dataset import SceneLoader, nuArgoDataset
    from trajsde_amd.scene_store import write_shard
    z = np.load(os.path.join(H.ROOT, "tests", "golden_data", "mixds.npz"))
    for sub, name, group in (("nu/val", "a", "raw/nus"), ("argo/train", "b", "raw/argo")):
        os.makedirs(tmp_path / sub)
        write_shard(str(tmp_path / sub / f"{name}.safetensors"), _groups(z, group))
    ds = nuArgoDataset("val", None, None, str(tmp_path / "nu"), str(tmp_path / "argo"), spec_args=BASE)
    loader = SceneLoader(ds, batch_size=6, device=dev)
    (host,) = list(loader._host_batches())
    return loader, host


def _first_batch_with_the_copy_stream_held(loader, monkeypatch):
    """(iterator, first batch, the hold's event): `torch.cuda.Stream`, as the loader's module sees it, hands out a stream that already
    carries a hold while the iterator creates its copy stream; restored before this returns"""
    from trajsde_amd import dataset as dataset_module
    held = []

    def held_stream(*a, **kw):
        s = torch.cuda.Stream(*a, **kw)
        held.append(ST.hold(s))
        return s
    monkeypatch.setattr(dataset_module, "torch", Through(torch, cuda=Through(torch.cuda, Stream=held_stream)))
    try:
        it = iter(loader)
        b = next(it)
    finally:
        monkeypatch.undo()
    assert dataset_module.torch is torch
    assert len(held) == 1 and b["x"].is_cuda
    return it, b, held[0]


def test_loader_hand_over_with_the_copy_stream_held(dev, tmp_path, monkeypatch):
    """SceneLoader copies a batch from pinned memory on a private stream; here that stream carries a hold from its creation on, so the
    copies have not started when the consumer's forward is enqueued: `_hand_over` must make the consumer's stream wait for them"""
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    loader, host = _scene_loader(tmp_path, dev)
    model = PredictionModelSDENet(**H.our_cfg(K, 60, 6.0), init_seed=5).eval().to(dev)
    want = serial(lambda: model(H.clone_batch(host).to(dev), noise=spec(77)))
    it, b, ev = _first_batch_with_the_copy_stream_held(loader, monkeypatch)
    with torch.no_grad():
        got = keep(model(b, noise=spec(77)))
    ST.assert_still_held(ev, "loader hand-over: the forward is enqueued while the copy stream waits behind the hold")
    torch.cuda.synchronize()
    ST.report(ev, "loader hand-over with the copy stream held")
    assert next(it, None) is None
    same(got, want, "forward of the loader's batch")


def test_loader_hand_over_under_plain_reads(dev, tmp_path, monkeypatch):
    """the same hand-over with the plainest consumer there is: every tensor of the batch copied on the consumer's stream, equal to the
    host batch.  (A consumer that dereferences nothing: what it reads too early can only be a wrong value.)"""
    loader, host = _scene_loader(tmp_path, dev)
    it, b, ev = _first_batch_with_the_copy_stream_held(loader, monkeypatch)
    got = {k: v.clone() for k, v in b.as_dict().items() if torch.is_tensor(v)}
    ST.assert_still_held(ev, "loader hand-over: the copies are enqueued while the copy stream waits behind the hold")
    torch.cuda.synchronize()
    ST.report(ev, "loader hand-over under plain reads")
    assert len(got) >= 10
    for k, v in got.items():
        assert torch.equal(v.cpu(), host[k]), k


# ------------------------------------------------------------------------------------------------------------ 8. replay beside eager
def test_graph_replays_beside_eager_forwards(dev, small, streams, main_model):
    """GraphedForward of one batch replayed from stream A while eager forwards of another batch run on B, six rounds without a
    synchronisation: every replay is the eager forward of its seed, every eager output the serial one"""
    from trajsde_amd import runtime
    A, B = streams[0], streams[1]
    model, _ = main_model
    want_g = [serial(lambda: model(on_device(small[0], dev), noise=spec(200 + r))) for r in range(6)]
    want_e = [serial(lambda: model(on_device(small[1], dev), noise=spec(300 + r))) for r in range(6)]
    gf = runtime.GraphedForward(model, on_device(small[0], dev))
    staged = [on_device(small[1], dev) for _ in range(6)]
    torch.cuda.synchronize()
    got_g, got_e = [], []
    with torch.no_grad():
        for r in range(6):
            with torch.cuda.stream(A):
                got_g.append(keep(gf(seed=200 + r)))
            with torch.cuda.stream(B):
                got_e.append(keep(model(staged[r], noise=spec(300 + r))))
    torch.cuda.synchronize()
    for r in range(6):
        same(got_g[r], want_g[r], ("replay", r))
        same(got_e[r], want_e[r], ("eager", r))


# ------------------------------------------------------------------------------------------------------------ 9. range guard
def test_range_guard_reports_under_overlap(dev, streams):
    """a forward whose decoder inputs pass the fp16 limit (test_gpu_range_guard's DEC_INPUT plant at 7e4) on A, a clean forward on B at
    the same time: trajsde_range_status names the planted site, B's output is the serial one"""
    import test_gpu_range_guard as RG
    A, B = streams[0], streams[1]
    planted, cfg, batch = RG.fresh_model("sde")
    RG.plant(planted, cfg, "dec_input", RG.OVER)
    planted = planted.to(dev)
    clean = RG.fresh_model("sde")[0].to(dev)
    want = serial(lambda: clean(on_device(batch, dev), noise=spec(RG.SEED)))
    with torch.no_grad():
        planted(on_device(batch, dev), noise=spec(RG.SEED))              # (images packed; its flags are cleared below)
    st, mask, _ = RG.read_flags(1)
    st, mask, _ = RG.read_flags(1)
    assert (st, mask) == (0, 0), RG.names_of(mask)
    ba, bb = on_device(batch, dev), on_device(batch, dev)
    with torch.no_grad():
        with torch.cuda.stream(A):
            planted(ba, noise=spec(RG.SEED))
        with torch.cuda.stream(B):
            got = keep(clean(bb, noise=spec(RG.SEED)))
    st, mask, msg = RG.read_flags(1)
    cell = RG.TABLE["DEC_INPUT"]["infer"]
    want_mask = RG.BIT["DEC_INPUT"]
    for e in cell.extra:
        want_mask |= RG.BIT[e]
    if not RG.fp16x3():
        want_mask = 0                                                     # a bf16x6 build has nothing to guard
    assert mask == want_mask, (RG.names_of(mask), RG.names_of(want_mask))
    if want_mask:
        assert st == RG.UNSUPPORTED and RG.WORDS["DEC_INPUT"] in msg, (st, msg)
    same(got, want, "clean forward beside the planted one")
