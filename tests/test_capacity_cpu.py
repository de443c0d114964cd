"""One static shape for any batch that fits (include/trajsde_hip_capacity.h, runtime.BatchCapacity / pad_batch_host /
CapacityBuffers), the parts that need no GPU: the extension header against `_lib.CAPACITY_EXT_SIGNATURES`, the exported symbols, the
capacity arithmetic and its messages, the refusals of the host side of trajsde_batch_pad, the host twin's padding rules, and -- the
premise of the whole feature -- that the padding is inert in the reference's semantics: `oracle/restate.forward` on a batch and on
its padded twin, under noise keyed by the unpadded row ids."""
import ctypes as C
import os
import re

import pytest
import torch

import helpers as H

NAMES = {"trajsde_batch_pad_fits", "trajsde_batch_pad"}
K, T = 3, 5


def test_capacity_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_capacity.h against `_lib.CAPACITY_EXT_SIGNATURES`, by the rules tests/test_cotangent_cpu.py applies to its header"""
    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    text = open(os.path.join(H.ROOT, "include", "trajsde_hip_capacity.h")).read()
    main = open(os.path.join(H.ROOT, "include", "trajsde_hip.h")).read()
    body = text.replace('#include "trajsde_hip.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.CAPACITY_EXT_SIGNATURES) == NAMES
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COT_SEL_EXT_SIGNATURES, _lib.GRID_EXT_SIGNATURES, _lib.CLIP_EXT_SIGNATURES,
                  _lib.ENC_COT_EXT_SIGNATURES):
        assert not set(_lib.CAPACITY_EXT_SIGNATURES) & set(other)
    assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", main))
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.CAPACITY_EXT_SIGNATURES, protos) == []
    swap = lambda tu: tu.replace('#include "trajsde_hip.h"', '#include "trajsde_hip_capacity.h"')
    r = CABI._compile_tu(swap(CABI._prototype_tu(_lib.CAPACITY_EXT_SIGNATURES, protos)), tmp_path, H.ROOT, "capacity")
    assert r.returncode == 0, r.stdout[-3000:]
    for name in NAMES:                                          # the check has teeth: one argument fewer is caught both ways
        bad = dict(_lib.CAPACITY_EXT_SIGNATURES)
        res, args = bad[name]
        bad[name] = (res, args[:-1])
        assert CABI._check_against_header(bad, protos)
        assert CABI._compile_tu(swap(CABI._prototype_tu(bad, protos)), tmp_path, H.ROOT, "capacity_bad").returncode != 0
    assert _lib.ABI_VERSION == 10 and _lib.lib().trajsde_abi_version() == 10   # an extension header: the ABI version did not move


def test_both_symbols_are_exported_by_the_built_library():
    from trajsde_amd import _lib
    lib = _lib.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.CAPACITY_EXT_SIGNATURES[name][1]
    assert lib.trajsde_abi_version() == 10


def test_the_staging_unit_forms_no_split_precision_product(tmp_path):
    """the range guard (csrc/range.hpp) notes the operands of the fp16x3 products; csrc/pad.hip has no site because it has no product:
    it includes neither the tile header nor the guard's, and its listing holds no matrix instruction"""
    import subprocess
    from trajsde_amd import build
    src = os.path.join(H.ROOT, "trajsde_amd", "csrc", "pad.hip")
    text = open(src).read()
    assert "tile.hpp" not in text and "range.hpp" not in text and "range_note" not in text
    out = tmp_path / "pad.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([build.HIPCC, *flags, "--cuda-device-only", "-S", "-o", str(out), src], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    assert "k_batch_pad" in asm and "global_store" in asm           # the scan looks at the kernel
    assert "mfma" not in asm


def _sizes(N, S, E, L, Ea):
    return {"actors": N, "scenes": S, "edges": E, "lanes": L, "lane_edges": Ea}


def test_batch_capacity_covering_fits_and_messages():
    from trajsde_amd.runtime import BatchCapacity
    from trajsde_amd.synth import synth
    a = synth(S=4, n=5, L=2, F=T, box=50.0, seed=1)            # N 20, S 4, E 80, L 8, E_al 40
    b = synth(S=1, n=12, L=3, F=T, box=50.0, seed=2)           # N 12, S 1, E 132, L 3, E_al 36
    assert BatchCapacity.sizes_of(a) == _sizes(20, 4, 80, 8, 40) and BatchCapacity.sizes_of(b) == _sizes(12, 1, 132, 3, 36)
    cap = BatchCapacity.covering([a, b])
    # every scene slot a batch leaves empty costs one pad actor: b needs 12 + (4 - 1) = 15 <= 20
    assert cap == BatchCapacity(actors=20, scenes=4, edges=132, lanes=8, lane_edges=40)
    assert cap.fits(a) and cap.fits(b) and cap.why_not(a) is None
    assert BatchCapacity.covering([_sizes(18, 1, 0, 0, 0), _sizes(4, 4, 0, 0, 0)]).actors == 21      # 18 + 3 pad scenes
    assert cap.padded_sizes() == (22, 5, 132, 9, 40)           # the reserve: two actors, one scene, one lane
    # N + (A_cap - S) <= N_cap, at and one past the bound
    assert cap.fits(_sizes(17, 1, 0, 0, 0)) and cap.fits(_sizes(20, 4, 132, 8, 40))
    assert not cap.fits(_sizes(18, 1, 0, 0, 0)) and not cap.fits(_sizes(20, 3, 0, 0, 0))
    for over, word in ((_sizes(21, 4, 0, 0, 0), "actors"), (_sizes(18, 1, 0, 0, 0), "actors"), (_sizes(5, 5, 0, 0, 0), "scenes"),
                       (_sizes(5, 1, 133, 0, 0), "edges"), (_sizes(5, 1, 0, 9, 0), "lanes"), (_sizes(5, 1, 0, 0, 41), "lane_edges")):
        why = cap.why_not(over)
        assert why is not None and why.startswith(word + ":"), (over, why)
    with pytest.raises(ValueError):
        BatchCapacity(actors=0, scenes=1, edges=0, lanes=0, lane_edges=0)
    with pytest.raises(ValueError):
        BatchCapacity.covering([])


def _fake_batch(sizes, H_=21, TT=26, P=10, null=()):
    """a trajsde_batch over stand-in addresses (never dereferenced: every call that gets one is refused on the host)"""
    from trajsde_amd import _lib
    fake = lambda i: 0x7F0000000000 + (i << 24)
    names = [n for n, t in _lib.Batch._fields_ if t is C.c_void_p]
    return _lib.Batch(*sizes, H_, TT, P, *[None if n in null else fake(k + 1) for k, n in enumerate(names)])


def test_batch_pad_refuses_before_any_launch():
    """an oversize source, mismatched time slots, null tables: refused by the host side with the dimension's name; no pointer is touched"""
    from trajsde_amd import _lib
    L = _lib.lib()
    p = 0x7E0000000000
    dst = _fake_batch((22, 5, 132, 9, 40))                      # capacity 20 actors, 4 scenes, 132 edges, 8 lanes, 40 lane edges
    tail = (3, 50.0, p, p, p, None)

    def call(src, dst_=dst, tail_=tail):
        fits = L.trajsde_batch_pad_fits(C.byref(src), C.byref(dst_))
        rc = L.trajsde_batch_pad(C.byref(src), p, T, C.byref(dst_), p, *tail_)
        return fits, rc, (L.trajsde_last_error() or b"").decode()

    assert L.trajsde_batch_pad_fits(C.byref(_fake_batch((20, 4, 132, 8, 40))), C.byref(dst)) == 0          # exactly at capacity
    assert L.trajsde_batch_pad_fits(C.byref(_fake_batch((17, 1, 0, 0, 0))), C.byref(dst)) == 0
    for sizes, word in (((21, 4, 0, 0, 0), "actors"), ((18, 1, 0, 0, 0), "actors"), ((5, 5, 0, 0, 0), "scenes"), ((5, 1, 133, 0, 0), "edges"),
                        ((5, 1, 0, 9, 0), "lanes"), ((5, 1, 0, 0, 41), "lane_edges")):
        fits, rc, msg = call(_fake_batch(sizes))
        assert fits == rc == -1 and f"batch_pad: {word}:" in msg, (sizes, msg)
    for kw, word in ((dict(TT=27), "TT"), (dict(H_=20), "H "), (dict(P=9), "lane_pts")):
        fits, rc, msg = call(_fake_batch((5, 1, 0, 0, 0), **kw))
        assert fits == rc == -1 and word in msg, (kw, msg)
    ok = _fake_batch((5, 1, 20, 2, 10))
    assert call(ok, tail_=(0, 50.0, p, p, p, None))[1] == -1                                             # num_modes
    for i in range(3):                                                                                   # a null row-id table
        t = list(tail)
        t[2 + i] = None
        assert call(ok, tail_=tuple(t))[1:] == (-1, "batch_pad: null row-id table")
    assert call(_fake_batch((5, 1, 20, 2, 10), null=("edge_index",)))[1] == -1
    assert call(ok, dst_=_fake_batch((22, 5, 132, 9, 40), null=("x",)))[1] == -1
    assert call(ok, dst_=_fake_batch((2, 5, 132, 9, 40)))[1] == -1                                       # a destination without the reserve
    assert L.trajsde_batch_pad_fits(None, C.byref(dst)) == -1


def _check_padding_rules(batch, cap, padded, ids, radius=50.0):
    """the rules of include/trajsde_hip_capacity.h, spelled out independently of pad_batch_host's arithmetic"""
    N, S = batch["x"].shape[0], batch["agent_index"].numel()
    E, L, Ea = batch["edge_index"].shape[1], batch["lane_positions"].shape[0], batch["lane_actor_index"].shape[1]
    Np, Ap, Ep, Lp, Eap = cap.padded_sizes()
    for k in ("x", "positions", "padding_mask", "bos_mask", "rotate_angles", "batch", "y"):
        assert padded[k].shape[0] == Np and torch.equal(padded[k][:N], batch[k]) and padded[k].dtype == batch[k].dtype, k
    assert bool(padded["padding_mask"][N:].all()) and not bool(padded["bos_mask"][N:].any())
    for k in ("x", "positions", "rotate_angles", "y"):
        assert not bool(padded[k][N:].any()), k
    ag, bt = padded["agent_index"], padded["batch"]
    assert ag.shape == (Ap,) and torch.equal(ag[:S], batch["agent_index"]) and bool((ag[1:] > ag[:-1]).all())
    assert bool((bt[1:] >= bt[:-1]).all()) and torch.equal(torch.unique(bt), torch.arange(Ap))           # every pad scene has an actor
    assert torch.equal(bt[ag], torch.arange(Ap))                                                         # ... and its agent is one of its own
    first = torch.tensor([int((bt == s).nonzero()[0]) for s in range(S, Ap)])
    assert torch.equal(ag[S:], first)                                                                    # ... its first
    assert not bool(padded["source"][S:].any()) and torch.equal(padded["source"][:S], batch["source"])
    perm = (bt == Ap - 1).nonzero().reshape(-1)                                                          # the permanent pad scene
    assert perm.numel() >= 2 and int(perm.min()) >= N
    ei = padded["edge_index"]
    assert ei.shape == (2, Ep) and torch.equal(ei[:, :E], batch["edge_index"])
    assert bool(torch.isin(ei[:, E:], perm).all()) and bool((ei[0, E:] != ei[1, E:]).all())
    if Ep > E:                                                                                           # dealt over the scene: no long row
        assert int(torch.bincount(ei[1, E:]).max()) <= -(-(Ep - E) // perm.numel())
    assert padded["lane_positions"].shape[0] == Lp and not bool(padded["lane_positions"][L:].any())
    assert padded["lane_paddings"].shape[0] == Lp and not bool(padded["lane_paddings"][L:].any())
    lai, lav = padded["lane_actor_index"], padded["lane_actor_vectors"]
    assert lai.shape == (2, Eap) and torch.equal(lai[:, :Ea], batch["lane_actor_index"]) and torch.equal(lav[:Ea], batch["lane_actor_vectors"])
    assert bool((lai[0, Ea:] == Lp - 1).all()) and bool(torch.isin(lai[1, Ea:], perm).all())
    assert bool((lav[Ea:].norm(dim=1) > 100 * radius).all()) and bool((lav[Ea:] == 200 * radius).all())  # from the radius, far outside it
    # row ids: real rows keep the ids of the unpadded batch, pad rows lie past them and nothing repeats
    fake, enc, dec = ids["fake_row_ids"].long(), ids["enc_row_ids"].long(), ids["dec_row_ids"].long().view(K, Np)
    assert all(v.dtype == torch.int32 for v in ids.values())
    assert torch.equal(fake[:S], torch.arange(S)) and fake.unique().numel() == Ap
    assert torch.equal(enc[:N], torch.arange(N)) and torch.equal(enc[Np:Np + S], N + torch.arange(S))
    assert enc.shape == (Np + Ap,) and enc.unique().numel() == Np + Ap
    assert torch.equal(dec[:, :N], torch.arange(K)[:, None] * N + torch.arange(N)[None, :])
    assert dec.unique().numel() == K * Np and int(dec[:, N:].min()) >= K * N


def _single_actor_batch():
    """two ordinary scenes and a single-actor scene (last: helpers._isolated_batch says why)"""
    from trajsde_amd.data import collate
    from trajsde_amd.synth import synth
    return collate([synth(S=1, n=6, L=3, F=T, box=50.0, seed=81, history_dropout=0.3), synth(S=1, n=5, L=2, F=T, box=50.0, seed=82, source=1),
                    synth(S=1, n=1, L=2, F=T, box=30.0, seed=83)])


def _cases():
    from trajsde_amd.synth import irregular, synth
    return {"dropout": lambda: synth(S=2, n=7, L=3, F=T, box=60.0, seed=5, history_dropout=0.3, mixed_source=True),
            "irregular": lambda: irregular(S=2, n=9, L=3, F=T, box=60.0, seed=6, mixed_source=True),
            "single_actor_scene": _single_actor_batch}


@pytest.fixture(scope="module")
def trained_model():
    model, cfg = H.build_model(K, T, 0.5, init_seed=3)
    H.trained_like_parameters(model, 17, 1.0)
    return model, cfg


@pytest.mark.parametrize("case", ["dropout", "irregular", "single_actor_scene"])
def test_padding_is_inert_in_the_oracle(case, trained_model):
    """restate.forward on a batch and on pad_batch_host's twin of it (+6 actors of which 2 are the reserve, +11 edges, +2 lanes,
    +5 lane edges, +1 scene and the permanent one), the twin under noise keyed by the unpadded row ids: the real rows of loc, pi,
    diff_in and diff_out agree within 1e-5 -- the project's bound for a scene's rows in another batch
    (test_scene_independence_of_the_oracle) -- and every pad row is finite"""
    import restate
    from trajsde_amd.runtime import BatchCapacity, pad_batch_host
    model, cfg = trained_model
    batch = _cases()[case]()
    s = BatchCapacity.sizes_of(batch)
    N, S = s["actors"], s["scenes"]
    cap = BatchCapacity(actors=N + 4, scenes=S + 1, edges=s["edges"] + 11, lanes=s["lanes"] + 1, lane_edges=s["lane_edges"] + 5)
    padded, ids = pad_batch_host(batch, cap, K, float(cfg["encoder"]["kwargs"]["local_radius"]))
    _check_padding_rules(batch, cap, padded, ids, float(cfg["encoder"]["kwargs"]["local_radius"]))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    seed = 123
    want = restate.forward(P, cfg, H.clone_batch(batch), restate.PhiloxNoise(seed))
    got = restate.forward(P, cfg, H.clone_batch(padded), restate.PhiloxNoise(seed, enc_row_ids=ids["enc_row_ids"].numpy(),
                                                                              dec_row_ids=ids["dec_row_ids"].numpy(),
                                                                              fake_row_ids=ids["fake_row_ids"].numpy()))
    diffs = {"loc": H.maxdiff(got["loc"][:, :N], want["loc"]), "pi": H.maxdiff(got["pi"][:N], want["pi"]),
             "diff_in": H.maxdiff(got["diff_in"][:S], want["diff_in"]), "diff_out": H.maxdiff(got["diff_out"][:S], want["diff_out"])}
    print(case, diffs)
    assert want["loc"].shape[1] == N and got["loc"].shape[1] == N + 6 and got["diff_in"].shape[0] == S + 2
    for k, v in diffs.items():
        assert v < 1e-5, (k, v)
    assert torch.equal(got["reg_mask"][:N], want["reg_mask"]) and not bool(got["reg_mask"][N:].any())
    for k in ("loc", "pi", "diff_in", "diff_out"):
        assert bool(torch.isfinite(got[k]).all()), k


def test_pad_batch_host_at_capacity_and_over_it():
    from trajsde_amd import _lib
    from trajsde_amd.runtime import BatchCapacity, pad_batch_host
    from trajsde_amd.synth import synth
    batch = synth(S=2, n=4, L=2, F=T, box=40.0, seed=9)
    cap = BatchCapacity.covering([batch])
    padded, ids = pad_batch_host(batch, cap, K)
    _check_padding_rules(batch, cap, padded, ids)                # it carries only the reserve: two actors, one scene, one lane
    assert padded["x"].shape[0] == 10 and padded["edge_index"].shape[1] == batch["edge_index"].shape[1]
    with pytest.raises(_lib.TrajsdeError, match="actors"):
        pad_batch_host(synth(S=1, n=8, L=2, F=T, box=40.0, seed=9), cap, K)       # 8 + one pad scene > 8


def test_capacity_buffers_refuse_the_host():
    """the staging launch has no CPU implementation: buffers on the host are refused, not emulated"""
    from trajsde_amd import _lib
    from trajsde_amd.runtime import BatchCapacity, CapacityBuffers
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        CapacityBuffers(BatchCapacity(actors=8, scenes=2, edges=24, lanes=4, lane_edges=16), K, "cpu", time_slots=21 + T)
    with pytest.raises(TypeError):
        CapacityBuffers((8, 2, 24, 4, 16), K, "cuda", time_slots=21 + T)
