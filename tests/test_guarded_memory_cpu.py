"""Self-test of tests/guarded_memory.py on CPU tensors: the helper catches what it claims to catch -- a one-byte write planted (with
ordinary torch indexing on the arena tensor) at interior_end, at interior_start - 1 and at the last guard byte is reported with the
right arena and offset, an untouched arena passes, a changed placed input is reported, and the pass-through rules hold."""
import pytest
import torch

import guarded_memory as GM

G = GM.GUARD_BYTES


def _three(gm):
    with gm:
        a = torch.empty(5, 64, device="cpu", dtype=torch.float32)
        b = torch.zeros(33, device="cpu", dtype=torch.uint8)
        c = torch.empty_like(a)
    return a, b, c


def test_layout_and_poison():
    assert G >= 64 * 1024 and G % 512 == 0
    with pytest.raises(ValueError):
        GM.GuardedMemory(guard_bytes=4096)
    with pytest.raises(ValueError):
        GM.GuardedMemory(guard_bytes=64 * 1024 + 100)
    for poison in ("nan", "zero", 7):
        gm = GM.GuardedMemory(poison=poison, route=("cpu",))
        a, b, c = _three(gm)
        assert gm.routed == 3 and len(gm.arenas) == 3
        assert a.shape == (5, 64) and a.dtype == torch.float32 and a.is_contiguous() and c.shape == a.shape
        for t, ar in zip((a, b, c), gm.arenas):
            assert ar.mem.numel() == G + ar.nbytes + G and ar.nbytes == t.numel() * t.element_size()
            assert t.data_ptr() == ar.interior_start == ar.mem.data_ptr() + G          # the tail guard starts where the request ends
            assert ar.interior_end == t.data_ptr() + ar.nbytes
            assert gm.owns(t) and gm.arena_of(t.data_ptr()) is ar
            assert bool((ar.mem[:G] == GM.CANARY).all()) and bool((ar.mem[G + ar.nbytes:] == GM.CANARY).all())
        assert bool((b == 0).all())                                                    # zeros are zeros under every poison
        if poison == "nan":
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(c).all())
            assert bool(torch.isnan(a.view(torch.bfloat16)).all()) and bool((a.view(torch.int32) == -1).all())
        elif poison == "zero":
            assert bool((a == 0).all())
        else:
            again = _three(GM.GuardedMemory(poison=poison, route=("cpu",)))[0]
            assert torch.equal(a.view(torch.int32), again.view(torch.int32)) and a.view(torch.int32).unique().numel() > 100
            assert not torch.equal(a.view(torch.int32), c.view(torch.int32))
        rep = gm.check()
        assert rep.ok and rep.n_arenas == 3, str(rep)                                  # untouched arenas pass


@pytest.mark.parametrize("where", ["interior_end", "interior_start-1", "last_guard_byte", "first_guard_byte"])
def test_planted_one_byte_write_is_reported_with_arena_and_offset(where):
    gm = GM.GuardedMemory(route=("cpu",))
    _three(gm)
    ar = gm.arenas[1]                                                                  # 33 bytes: the tail guard is not word aligned
    at, side, off = {"interior_end": (G + ar.nbytes, "tail", 0), "interior_start-1": (G - 1, "lead", -1),
                     "last_guard_byte": (G + ar.nbytes + G - 1, "tail", G - 1), "first_guard_byte": (0, "lead", -G)}[where]
    ar.mem[at] = ar.mem[at] ^ 1
    rep = gm.check()
    assert not rep.ok and not rep.changed and len(rep.hits) == 1
    hit = rep.hits[0]
    assert hit[0] is ar and hit[1:] == (side, off, 1), rep.hits
    assert "zeros(33,)" in str(rep) and "test_guarded_memory_cpu.py" in str(rep) and "_three" in str(rep)      # which arena, allocated where


@pytest.mark.parametrize("fill", ["A", "B"])
def test_placed_inputs(fill):
    gm = GM.GuardedMemory(route=("cpu",))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 21, 2, generator=g)
    ei = torch.randint(0, 7, (2, 13), generator=g)
    mask = torch.rand(7, 21, generator=g) < 0.3
    px, pe, pm = gm.placed(x, fill), gm.placed(ei, fill), gm.placed(mask, fill)
    for src, p, ar in zip((x, ei, mask), (px, pe, pm), gm.arenas):
        assert p.dtype == src.dtype and p.shape == src.shape and p.is_contiguous() and torch.equal(p, src)
        assert p.data_ptr() == ar.interior_start and p.data_ptr() != src.data_ptr() and ar.kind == "placed"
        guards = torch.cat([ar.mem[:G], ar.mem[G + ar.nbytes:]]).view(torch.uint8 if src.dtype == torch.bool else src.dtype)
        if src.is_floating_point():
            assert bool(torch.isnan(guards).all()) if fill == "A" else bool((guards == 1e30).all())
        else:
            assert bool((guards == (0 if fill == "A" else 1)).all())                  # legal ids / mask bytes, never a bit pattern
    assert gm.check().ok
    empty = gm.placed(torch.zeros(2, 0, dtype=torch.int64), fill)                      # E = 0: the guards meet
    assert empty.shape == (2, 0) and gm.arenas[-1].nbytes == 0 and gm.check().ok
    pe[1, 12] += 1                                                                     # inputs are const in the ABI
    rep = gm.check()
    assert not rep.ok and not rep.hits and len(rep.changed) == 1
    assert rep.changed[0][0] is gm.arenas[1] and rep.changed[0][1] == (13 + 12) * 8 and "INPUT CHANGED" in str(rep)
    gm.arenas[0].mem[G + gm.arenas[0].nbytes] ^= 0xFF                                    # an overrun past a placed float input
    rep = gm.check()
    assert len(rep.hits) == 1 and rep.hits[0][0] is gm.arenas[0] and rep.hits[0][1:3] == ("tail", 0)
    with pytest.raises(TypeError):
        gm.placed(torch.zeros(3, dtype=torch.int32))


def test_pass_through_rules():
    before = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like)
    gm = GM.GuardedMemory()                                                            # routes device memory only
    with gm:
        assert torch.empty is not before[0]
        a = torch.empty(8, device="cpu")
        b = torch.zeros(3, 3)                                                          # no device argument: the host
        c = torch.empty_like(a)
        with pytest.raises(RuntimeError):
            GM.GuardedMemory().__enter__()                                             # one context at a time
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == before   # restored
    assert gm.routed == 0 and not gm.arenas and gm.passed == 3 and not gm.owns(a) and not gm.owns(c) and bool((b == 0).all())
    gm = GM.GuardedMemory(route=("cpu",))
    outside = torch.empty(8, device="cpu")                                             # outside the context
    strided = torch.zeros(4, 6, device="cpu").t()
    with gm:
        z = torch.empty(0, dtype=torch.int32, device="cpu")                            # zero-byte requests keep their behaviour
        z2 = torch.empty(4, 0, device="cpu")
        nc = torch.empty_like(strided)                     # a layout this module does not model
        default = torch.empty(4)                                                       # no device named
        sized = torch.empty((2, 3), device="cpu", dtype=torch.int32)                  # a size tuple is a size
        inside = torch.zeros_like(outside)
    after = torch.empty(8, device="cpu")
    assert z.numel() == 0 and z2.shape == (4, 0) and nc.shape == (6, 4)
    for t in (outside, z, z2, nc, default, after):
        assert not gm.owns(t)
    assert gm.owns(sized) and gm.owns(inside) and gm.routed == 2 and sized.dtype == torch.int32 and bool((inside == 0).all())
    assert not gm.owns(None) and gm.arena_of(sized.data_ptr(), 24) is not None and gm.arena_of(sized.data_ptr(), 25) is None
    try:
        with gm:
            raise KeyError("x")
    except KeyError:
        pass
    assert torch.empty is before[0] and GM.GuardedMemory._active is None               # restored when the body raises
