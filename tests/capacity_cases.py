"""Shared by tests/test_gpu_capacity.py and tests/test_gpu_capacity_memory.py: the batches, a poisoned set of static buffers, and the
staging launch (trajsde_batch_pad) called on them directly -- no model."""
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


def single_actor_first():
    return _collate([_synth(S=1, n=1, L=2, F=T, box=30.0, seed=210), _synth(S=1, n=9, L=3, F=T, box=60.0, seed=211),
                     _synth(S=1, n=6, L=2, F=T, box=50.0, seed=212, source=1)])


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
