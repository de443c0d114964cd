"""The fused edge attention with the last LayerNorm's scale folded through lin_k | lin_v (-m gpu; csrc/attn.hip k_edge_attn2 FOLD,
csrc/layouts.hpp EdgeL6F MKV | CKV0): the AA and the AL edge-attention blocks, run through the encoder's C-ABI entry point, against the
float64 oracle of tests/helpers.py on graphs that put the kernel's row streams through their edge cases.

The yardstick is the error of the build BEFORE the fold (the parent commit, which split the normalised embedding rows and multiplied them
by lin_k | lin_v) against the same oracle on the same inputs, measured once on that build with this file's `_errors` and recorded in
PARENT below (and in profiles/r08_edge_fold.md beside this build's figures).  The fold re-associates one 64-term product; its error class
is the parent's (a 2^-22-class operand error, amplified alike by rstd in both forms).  Each case asserts

    error <= 2 x the parent's error of that quantity   and   error <= 1e-4, the bound of tests/test_gpu_trained_weights.py for it,

where "error" is max |got - oracle| / max(1, max |oracle|) of aa_out [H, Nt, 64] (the AA block's output) and of local_embed [N, 64]
(the AL block's output, behind the recurrence).

Figures (max error, parent -> this build, one MI355X):
    three_actors                 aa_out 5.91e-07 -> 5.11e-07   local_embed 6.25e-07 -> 6.24e-07
    seventeen_actors             aa_out 7.01e-07 -> 6.04e-07   local_embed 6.64e-07 -> 6.15e-07
    thirtythree_actors           aa_out 6.01e-07 -> 6.17e-07   local_embed 6.88e-07 -> 6.53e-07
    actor_outside_every_radius   aa_out 6.32e-07 -> 6.98e-07   local_embed 6.65e-07 -> 5.88e-07
    mixed_sources                aa_out 6.88e-07 -> 6.88e-07   local_embed 7.63e-07 -> 7.03e-07
    trained_mixed_k6_t20         aa_out 7.12e-07 -> 6.38e-07   local_embed 8.80e-07 -> 8.54e-07
    flat_embedding_rstd          aa_out 1.74e-06 -> 1.10e-06   local_embed 3.19e-06 -> 1.86e-06
"""
import numpy as np
import pytest
import torch

import edge_fold_twin as T
import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # tests/test_gpu_trained_weights.py TOL for aa_out / local_embed
SEED = 6
K, FUT, MAX_T = 6, 20, 2.0

# the parent build's errors: case -> (aa_out, local_embed)
PARENT = {
    "three_actors": (5.906e-07, 6.246e-07),
    "seventeen_actors": (7.005e-07, 6.643e-07),
    "thirtythree_actors": (6.013e-07, 6.879e-07),
    "actor_outside_every_radius": (6.316e-07, 6.645e-07),
    "mixed_sources": (6.877e-07, 7.626e-07),
    "trained_mixed_k6_t20": (7.119e-07, 8.801e-07),
    "flat_embedding_rstd": (1.741e-06, 3.193e-06),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trajsde_amd import _lib
    _lib.lib()          # a missing/broken HIP library is a failure, not a skip
    return torch.device("cuda:0")


def _synth(**kw):
    from trajsde_amd.synth import synth
    return synth(**kw)


def _outside_batch():
    """a 12-actor scene with one actor moved 1000 m away at every step: no edge reaches it or leaves it, so its rows never flush a
    record (and the AL block finds no lane for it)"""
    b = _synth(S=1, n=12, L=5, F=FUT, box=40.0, seed=83)
    far = 3
    assert far not in set(int(i) for i in b["agent_index"])
    b["positions"][far] += 1000.0
    keep = b["lane_actor_index"][1] != far
    b["lane_actor_index"], b["lane_actor_vectors"] = b["lane_actor_index"][:, keep], b["lane_actor_vectors"][keep]
    return b


def _weights_plain(model):
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)


def _weights_flat_embedding(model):
    """the rstd amplification case: the second layer of both embeddings (aggr_embed.2, the layer in front of the folded LayerNorm)
    scaled by 0.05, so that the centred embedding row is nearly constant over its features and rstd is up to 20 x larger"""
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in ("encoder.aa_encoder.nbr_embed", "encoder.al_encoder.lane_embed"):
            params[emb + ".aggr_embed.2.weight"].mul_(0.05)
            params[emb + ".aggr_embed.2.bias"].mul_(0.05)


# name -> (batch maker, weights, largest AA in-degree expected or None)
CASES = {
    "three_actors": (lambda: _synth(S=1, n=3, L=4, F=FUT, box=20.0, seed=81), _weights_plain, 2),
    "seventeen_actors": (lambda: _synth(S=1, n=17, L=6, F=FUT, box=40.0, seed=82), _weights_plain, 16),
    "thirtythree_actors": (lambda: _synth(S=1, n=33, L=6, F=FUT, box=45.0, seed=84), _weights_plain, 32),
    "actor_outside_every_radius": (_outside_batch, _weights_plain, None),
    "mixed_sources": (lambda: _synth(S=3, n=14, L=6, F=FUT, box=70.0, seed=85, mixed_source=True), _weights_plain, None),
    "trained_mixed_k6_t20": (H.TRAINED_CASES["mixed_k6_t20"][3], _weights_plain, None),
    "flat_embedding_rstd": (lambda: _synth(S=2, n=17, L=6, F=FUT, box=50.0, seed=86, mixed_source=True), _weights_flat_embedding, None),
}
_CACHE = {}


def _model(weights):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    cfg = H.our_cfg(K, FUT, MAX_T)
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    weights(model)
    return model, cfg


def _case(name):
    """(cfg, batch, weights, float64 oracle with intermediates), the oracle computed once per case and left alone"""
    if name not in _CACHE:
        make, weights, deg = CASES[name]
        model, cfg = _model(weights)
        batch = make()
        want = H.oracle_forward64(model, cfg, batch, noise_seed=SEED)
        _CACHE[name] = (cfg, batch, weights, want, deg)
    return _CACHE[name]


def _scaled(a, ref):
    return H.maxdiff(a, ref) / max(1.0, float(ref.abs().max()))


def _run_encoder(model, batch, dev):
    from trajsde_amd.runtime import NoiseSpec, rotate_inputs
    data = H.clone_batch(batch).to(dev)
    data["rotate_mat"], _ = rotate_inputs(data)
    model.encoder.capture_intermediates = True
    with torch.no_grad():
        local = model.encoder(data=data, noise=NoiseSpec(seed=SEED))[0]
    torch.cuda.synchronize()
    return model.encoder.last_intermediates["aa_out"].cpu(), local.cpu(), model.encoder.last_intermediates


def _errors(name, dev):
    """(aa_out error, local_embed error) of the loaded library on case `name` -- also what measured PARENT, with the parent's library"""
    from trajsde_amd import _lib
    cfg, batch, weights, want, deg = _case(name)
    model, _ = _model(weights)
    aa, local, im = _run_encoder(model.to(dev), batch, dev)
    _lib.check_range()
    assert im["E_aa"] == want["aa_edges"]
    return _scaled(aa, want["aa_out"]), _scaled(local, want["local_embed"])


def test_cases_are_the_graphs_they_claim_to_be():
    """in-degrees of the oracle's edge lists (no GPU work): 2 edges per target; 16 and 32; a target without any edge next to targets
    with edges; both sources and fake-agent rows present"""
    for name, (_, _, deg) in CASES.items():
        cfg, batch, _, want, _ = _case(name)
        N, A = batch["x"].shape[0], batch["agent_index"].shape[0]
        Nt, Hs = N + A, int(want["aa_out"].shape[0])
        indeg = torch.bincount(want["aa_edge_list"][1], minlength=Hs * Nt).view(Hs, Nt)
        assert A > 0 and int(indeg[:, N:].max()) > 0, name          # fake-agent rows receive edges
        if deg is not None:
            assert int(indeg.max()) == deg, (name, int(indeg.max()))
        if name == "three_actors":
            assert set(indeg[-1, :N].tolist()) == {2}, indeg[-1]
        if name == "actor_outside_every_radius":
            assert int(indeg[:, 3].max()) == 0 and int(indeg[-1].max()) >= 8
            assert int((want["al_edge_list"][1] == 3).sum()) == 0 and want["al_edge_list"].shape[1] > 0
        if name in ("mixed_sources", "trained_mixed_k6_t20", "flat_embedding_rstd"):
            assert set(batch["source"].tolist()) == {0, 1}, name


@pytest.mark.parametrize("name", list(CASES))
def test_edge_attention_blocks_match_float64_oracle_within_twice_the_parent(name, dev):
    aa, local = _errors(name, dev)
    p_aa, p_local = PARENT[name]
    print(f"[edge-fold] {name}: aa_out {aa:.3e} (parent {p_aa:.3e}), local_embed {local:.3e} (parent {p_local:.3e})")
    assert aa <= 2 * p_aa and aa <= TOL, (name, aa, p_aa)
    assert local <= 2 * p_local and local <= TOL, (name, local, p_local)


def test_a_run_and_its_repeat_agree_bit_for_bit(dev):
    cfg, batch, weights, want, _ = _case("mixed_sources")
    model, _ = _model(weights)
    model = model.to(dev)
    a0, l0, _ = _run_encoder(model, batch, dev)
    a1, l1, _ = _run_encoder(model, batch, dev)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(l0).all())


@pytest.mark.parametrize("weights", [_weights_plain, _weights_flat_embedding])
def test_packed_image_is_the_float64_composite(weights, dev):
    """MKV | CKV0 of both blocks in the packed encoder blob against the float64 twin of the pack jobs: every matrix element the kernel
    multiplies by (hi + lo of its two fp16 pieces, read in fragment order) within the 22 bits of the split plus the fp32 rounding, the
    constants within an fp32 rounding -- an image split from an fp32 product of split pieces would miss this by 2^-11"""
    from trajsde_amd import _lib
    if _lib.lib().trajsde_split_products() != 3:
        pytest.skip("the fused edge attention exists in the fp16x3 build only")
    model, _ = _model(weights)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    blob = model.encoder._rt.blob().detach().cpu().numpy()
    assert blob.dtype == np.float32
    off = _lib.edge_fold_offsets(blob.size)
    for block in ("aa", "al"):
        wk, wv, gamma, w2, b2 = T.block_parameters(sd, block)
        words = blob[off[block]:off[block] + _lib.EDGE_FOLD_IMAGE_FLOATS]
        for h, W in enumerate((wk, wv)):
            M, c = T.composite(W, gamma, w2, b2)
            got = T.matrix_of_image(words[4096 * h:4096 * (h + 1)].view(np.uint16))
            # (+ 2^-25: a low piece below 2^-14 is an fp16 subnormal, spaced 2^-24 -- csrc/range.hpp)
            assert np.abs(got - M).max() <= (2.0 ** -21 + 2.0 ** -24) * np.abs(M).max() + 2.0 ** -25, (block, h)
            got_c = words[8192 + 64 * h:8192 + 64 * (h + 1)].astype(np.float64)
            assert np.abs(got_c - c).max() <= 2.0 ** -23 * np.abs(c).max(), (block, h)
        want_words = T.fold_image(wk, wv, gamma, w2, b2)
        same = float(np.mean(words.view(np.uint32) == want_words.view(np.uint32)))
        assert same >= 0.999, (block, same)                      # word for word, but for roundings at a double-precision tie
