"""trajsde_batch_pad inside the red-zone arenas of tests/guarded_memory.py (-m gpu): the accounting of tests/test_gpu_clip_memory.py for
`_lib.CAPACITY_EXT_SIGNATURES`.  Every source tensor in an arena of its own (guards filled with values legal for its role, interior
compared with a snapshot: sources are read only inside their tensors and never written); every destination tensor and table routed into
an arena that starts as NaN, as zeros or as random bits (destinations are written only inside theirs, and in full: the result is the
host twin's under all three)."""
import pytest
import torch

import capacity_cases as CC
import guarded_memory as GM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def test_every_capacity_entry_point_is_a_host_query_or_runs_in_these_arenas():
    from trajsde_amd import _lib
    assert set(_lib.CAPACITY_EXT_SIGNATURES) == {"trajsde_batch_pad_fits", "trajsde_batch_pad"}     # `_fits` launches nothing


@pytest.mark.parametrize("name", ["n17", "n33", "at_capacity", "no_edges", "no_lanes"])
def test_batch_pad_stays_inside_its_buffers(name, dev):
    from trajsde_amd.data import TemporalData
    batch = CC.STAGING[name]()
    cap = CC.capacity()
    for fill, poison in (("A", "nan"), ("B", "zero"), ("A", 7)):
        gm = GM.GuardedMemory(poison=poison)
        placed = {}
        for k, v in batch.as_dict().items():
            if torch.is_tensor(v):
                v = v.to(dev)
                placed[k] = gm.placed(v, fill, label=k) if v.numel() else v
            else:
                placed[k] = v
        n_src = len(gm.arenas)
        with gm:
            static, ids = CC.poisoned_static(cap, dev, byte=None)
        dests = [v for v in static.as_dict().values() if torch.is_tensor(v)] + list(ids.values())
        assert len(dests) == 14 + 3 and gm.routed == len(dests) and all(gm.owns(t) for t in dests)
        assert len(gm.arenas) == n_src + len(dests)
        assert CC.stage(TemporalData(**placed), static, ids) == 0
        torch.cuda.synchronize()
        rep = gm.check()
        assert rep.ok, f"{name} poison={poison}\n{rep}"                 # guards intact, sources unchanged
        CC.assert_is_twin(static, ids, batch, cap, f"{name} {poison}")  # written in full: nothing of the poison is left
