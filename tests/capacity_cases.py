"""Shared by tests/test_gpu_capacity.py and tests/test_gpu_capacity_memory.py: the batches, a poisoned set of static buffers, and the
staging launch (trajsde_batch_pad) called on them directly -- no model.  And by tests/test_capacity_edges_cpu.py and
tests/test_gpu_capacity_edges.py: the batches whose padding concentrates on two actors, with their preconditions."""
import ctypes as C

import torch

K, T = 3, 6
RADIUS = 50.0


def _synth(**kw):
    from trajsde_amd.synth import synth
    return synth(**kw)


def _collate(scenes):
    from trajsde_amd.data import collate
    return collate(scenes)


def full_batch():
    """64 actors in 5 scenes of 40, 6, 6, 6, 6 with 16 lanes: BatchCapacity.covering([full_batch()]) is the capacity of these tests, and
    this batch then carries nothing but the reserve"""
    return _collate([_synth(S=1, n=n, L=L, F=T, box=70.0, seed=200 + i, source=i % 2)
                     for i, (n, L) in enumerate(((40, 4), (6, 3), (6, 3), (6, 3), (6, 3)))])


def single_actor_first_scenes():
    return [_synth(S=1, n=1, L=2, F=T, box=30.0, seed=210), _synth(S=1, n=9, L=3, F=T, box=60.0, seed=211),
            _synth(S=1, n=6, L=2, F=T, box=50.0, seed=212, source=1)]


def single_actor_first():
    return _collate(single_actor_first_scenes())


# what the staging launch is compared on, bit for bit: actors one below, at, one above a 16-row tile and over two tiles (several
# workgroups' worth of edge columns), no edge at all, no lane at all
STAGING = {
    "n15": lambda: _synth(S=1, n=15, L=4, F=T, box=60.0, seed=55, history_dropout=0.3),
    "n16": lambda: _synth(S=2, n=8, L=4, F=T, box=60.0, seed=56, mixed_source=True),
    "n17": lambda: _synth(S=1, n=17, L=4, F=T, box=60.0, seed=57),
    "n33": lambda: _synth(S=3, n=11, L=4, F=T, box=60.0, seed=58, mixed_source=True),
    "at_capacity": full_batch,
    "no_edges": lambda: _collate([_synth(S=1, n=1, L=2, F=T, box=30.0, seed=60 + i) for i in range(3)]),
    "no_lanes": lambda: _synth(S=2, n=6, L=0, F=T, box=60.0, seed=59),
}


def capacity():
    from trajsde_amd.runtime import BatchCapacity
    cap = BatchCapacity.covering([full_batch()])
    assert cap == BatchCapacity(actors=64, scenes=5, edges=1680, lanes=16, lane_edges=232)
    return cap


# ---------------------------------------------------------------------------------------------- concentrated padding
# (tests/test_capacity_edges_cpu.py, tests/test_gpu_capacity_edges.py).  A batch that fills the ACTOR capacity leaves the permanent
# pad scene its two reserve actors, and every pad edge (lane-actor edge) lands on those two: CSR rows of (edges - E) / 2 copies of
# ONE sender, which the graph stage sorts in LDS past 256 entries and in global memory past 4096.
def _scene_list(ns, L, box, seed, alternate_source=False):
    return [_synth(S=1, n=n, L=L, F=T, box=box, seed=seed + i, **({"source": i % 2} if alternate_source else {})) for i, n in enumerate(ns)]


def _scenes(*a, **kw):
    return _collate(_scene_list(*a, **kw))


def lds_rows_scenes():
    return _scene_list((13, 13, 13, 13, 12), 3, 60.0, 300, alternate_source=True)


def _lds_rows():
    return capacity(), _collate(lds_rows_scenes())


def _global_rows():
    from trajsde_amd.runtime import BatchCapacity
    return BatchCapacity.covering([_scenes((116, 1, 1, 1, 1), 3, 120.0, 400)]), _scenes((24,) * 5, 3, 60.0, 500)


def _lane_rows():
    """no lane at all in the batch, 532 lane-actor edges in the capacity: 266 pad lane-actor edges per pad actor"""
    from trajsde_amd.runtime import BatchCapacity
    batch = _synth(S=2, n=10, L=0, F=T, box=60.0, seed=600)
    return BatchCapacity.covering([_synth(S=1, n=19, L=28, F=T, box=60.0, seed=601), batch]), batch


# name -> (builder of (capacity, batch), what pad_batch_host's twin must show: the capacity, the batch's actors and edges, the pad
# in-degree of each of the two pad actors in the actor graph and in the lane graph)
CONCENTRATED = {
    "lds_rows": (_lds_rows, dict(cap=(64, 5, 1680, 16, 232), actors=64, edges=756, pad_in=462, pad_lane_in=None)),
    "global_rows": (_global_rows, dict(cap=(120, 5, 13340, 15, 360), actors=120, edges=2760, pad_in=5290, pad_lane_in=None)),
    "lane_rows": (_lane_rows, dict(cap=(20, 2, 342, 28, 532), actors=20, edges=180, pad_in=81, pad_lane_in=266)),
}
WAVE_SORT_MAX, LDS_SORT_MAX = 256, 4096          # csrc/prep.hip: rows up to 256 entries in one wave, up to 4096 in LDS, longer in global memory


def sort_path(n):
    return "wave" if n <= WAVE_SORT_MAX else "lds" if n <= LDS_SORT_MAX else "global"


def concentrated(name, radius=RADIUS):
    """(capacity, batch, pad_batch_host's twin, its row ids) of a CONCENTRATED case, its preconditions asserted on the host: a later
    change of synth cannot turn the case into a vacuous one"""
    from trajsde_amd import runtime
    build, want = CONCENTRATED[name]
    cap, batch = build()
    assert (cap.actors, cap.scenes, cap.edges, cap.lanes, cap.lane_edges) == want["cap"], (name, cap)
    assert cap.fits(batch), cap.why_not(batch)
    sizes = runtime.BatchCapacity.sizes_of(batch)
    N, S = sizes["actors"], sizes["scenes"]
    assert (N, sizes["edges"]) == (want["actors"], want["edges"]), (name, sizes)
    assert N + (cap.scenes - S) == cap.actors                            # the actor capacity is full ...
    twin, ids = runtime.pad_batch_host(batch, cap, K, radius)
    Np, Ap = cap.padded_sizes()[:2]
    perm = (twin["batch"] == Ap - 1).nonzero().reshape(-1)
    assert perm.tolist() == [Np - 2, Np - 1] and int(perm.min()) >= N     # ... so the permanent pad scene is the reserve: 2 actors
    ei, lai = twin["edge_index"], twin["lane_actor_index"]
    E, Ea = sizes["edges"], sizes["lane_edges"]
    assert bool(torch.isin(ei[:, E:], perm).all()) and bool(torch.isin(lai[1, Ea:], perm).all())
    deg = torch.bincount(ei[1], minlength=Np)
    assert deg[perm].tolist() == [want["pad_in"]] * 2 and 2 * want["pad_in"] == cap.edges - E, (name, deg[perm])
    for p in perm.tolist():                                               # a row of ONE duplicated sender: the other pad actor
        assert torch.unique(ei[0, ei[1] == p]).tolist() == [Np - 1 + Np - 2 - p]
    assert int(deg[:N].max()) <= WAVE_SORT_MAX                            # the long rows are the padding's alone
    lane_deg = torch.bincount(lai[1], minlength=Np)
    assert lane_deg[perm].tolist() == [(cap.lane_edges - Ea) // 2] * 2
    if name == "lds_rows":
        assert sort_path(want["pad_in"]) == "lds" and 256 < want["pad_in"] <= 512          # padded to 512 in LDS
    if name == "global_rows":
        assert sort_path(want["pad_in"]) == "global" and want["pad_in"] & (want["pad_in"] - 1)   # ... and no power of two
    if name == "lane_rows":
        assert sizes["lanes"] == 0 and Ea == 0 and int(lane_deg[perm].min()) == want["pad_lane_in"]
        assert sort_path(want["pad_lane_in"]) == "lds" and sort_path(want["pad_in"]) == "wave"
    return cap, batch, twin, ids


def embedded_ids(N, S, N2, S2, num_modes=K):
    """row-id tables under which the first N actors / S scenes of a batch of N2 actors / S2 scenes draw the noise of the batch of N
    actors and S scenes alone -- the rule of include/trajsde_hip_capacity.h, spelled out once more: what pad_batch_host returns for
    its twin, and what puts the same scenes inside ANOTHER real batch (the scene-independence comparison)"""
    i = torch.arange(N2 + S2)
    enc = torch.where(i < N, i, torch.where(i < N2, i + S, torch.where(i - N2 < S, N + (i - N2), i)))
    n, k = torch.arange(N2)[None, :], torch.arange(num_modes)[:, None]
    dec = torch.where(n < N, k * N + n, num_modes * N + k * (N2 - N) + (n - N))
    return {"fake_row_ids": torch.arange(S2, dtype=torch.int32), "enc_row_ids": enc.to(torch.int32), "dec_row_ids": dec.reshape(-1).to(torch.int32)}


def poisoned_static(cap, dev, TT=21 + T, lane_pts=10, byte=0xA5, alloc=None):
    """(static batch, row-id tables) of the capacity's padded sizes on `dev` with EVERY byte set to `byte` (masks included: bool
    tensors over arbitrary bytes, compared as bytes); `alloc(shape, dtype)`: where the tensors come from (default torch.empty); `byte` None: left as allocated"""
    from trajsde_amd import runtime
    twin, ids = runtime.pad_batch_host(runtime._empty_batch(21, TT, lane_pts), cap, K, RADIUS)
    alloc = alloc or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))

    def like(t):
        out = alloc(tuple(t.shape), torch.uint8 if t.dtype == torch.bool else t.dtype)
        if out.numel() and byte is not None:
            out.view(-1).view(torch.uint8).fill_(byte)
        return out.view(torch.bool) if t.dtype == torch.bool else out

    from trajsde_amd.data import TemporalData
    static = TemporalData(**{k: (like(v) if torch.is_tensor(v) else v) for k, v in twin.as_dict().items()})
    return static, {k: like(v) for k, v in ids.items()}


def stage(batch_dev, static, ids, radius=RADIUS, num_modes=K):
    """trajsde_batch_pad of a device batch into `static` / `ids` on the current stream -> the status"""
    from trajsde_amd import _lib, runtime
    keep = []
    src, dst = runtime._c_batch(batch_dev, keep=keep), runtime._c_batch(static, keep=keep)
    src.lane_pts = dst.lane_pts
    y = batch_dev.y
    F = static.y.shape[1]
    rc = _lib.lib().trajsde_batch_pad(C.byref(src), None if y is None else y.data_ptr(), F, C.byref(dst), static.y.data_ptr(), num_modes,
                                      radius, ids["fake_row_ids"].data_ptr(), ids["enc_row_ids"].data_ptr(), ids["dec_row_ids"].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    return rc


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def assert_is_twin(static, ids, batch_host, cap, tag=""):
    """every destination tensor and all three tables against runtime.pad_batch_host, byte for byte"""
    from trajsde_amd import runtime
    twin, twin_ids = runtime.pad_batch_host(batch_host, cap, K, RADIUS)
    names = [k for k, v in twin.as_dict().items() if torch.is_tensor(v)]
    assert set(names) == {"x", "positions", "padding_mask", "bos_mask", "rotate_angles", "edge_index", "agent_index", "batch", "source",
                          "lane_positions", "lane_paddings", "lane_actor_index", "lane_actor_vectors", "y"}
    for k in names:
        got, want = static[k], twin[k]
        assert got.shape == want.shape and got.dtype == want.dtype, (tag, k, got.shape, want.shape)
        assert torch.equal(_bytes(got).cpu(), _bytes(want)), (tag, k)
    for k, want in twin_ids.items():
        assert torch.equal(ids[k].cpu(), want), (tag, k)
