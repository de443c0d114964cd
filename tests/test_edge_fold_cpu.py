"""The folded key / value image of the fused edge attention (csrc/layouts.hpp EdgeL6F MKV | CKV0, csrc/pack.hip PK_MAT6_FOLD), the
parts that need no GPU: the algebra of the fold in float64 (tests/edge_fold_twin.py, the twin of the pack jobs) at random weights and at
the trained-like profile, the fragment layout of the twin's image read back from the consumer's side, and the Python binding of the
image's place in the encoder blob.  tests/test_gpu_edge_fold.py compares the packed blob with the same twin."""
import re

import numpy as np
import pytest
import torch

import edge_fold_twin as T
import helpers as H


def _reference_kv(W, b, gamma, beta, w2, b2, h):
    """W LN(W2 h + b2) + b in float64, the LayerNorm spelled out (eps 1e-5, biased variance) -> (value, rstd)"""
    y = w2 @ h + b2
    yc = y - y.mean()
    rstd = 1.0 / np.sqrt((yc * yc).mean() + 1e-5)
    return W @ (gamma * yc * rstd + beta) + b, rstd


def _random_case(seed):
    g = np.random.default_rng(seed)
    W, w2 = g.normal(size=(64, 64)) / 8, g.normal(size=(64, 64)) / 8
    return W, g.normal(size=64), 1 + 0.4 * g.normal(size=64), g.normal(size=64), w2, g.normal(size=64)


def _trained_cases():
    model, _ = H.build_model(6, 20, 2.0, init_seed=2)
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    sd = model.state_dict()
    for block, att, emb in (("aa", "encoder.aa_encoder", "encoder.aa_encoder.nbr_embed"), ("al", "encoder.al_encoder", "encoder.al_encoder.lane_embed")):
        wk, wv, gamma, w2, b2 = T.block_parameters(sd, block)
        beta = sd[emb + ".aggr_embed.3.bias"].double().numpy()
        for W, b in ((wk, sd[att + ".lin_k.bias"]), (wv, sd[att + ".lin_v.bias"])):
            yield block, (W, b.double().numpy(), gamma, beta, w2, b2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fold_is_the_layer_behind_the_layernorm_at_random_weights(seed):
    """rstd (M h' + c) + (W beta + b) == W LN(W2 h' + b2) + b, and without rstd: M h' + c == W diag(gamma) (W2c h' + b2c), to 1e-12"""
    W, b, gamma, beta, w2, b2 = _random_case(seed)
    M, c = T.composite(W, gamma, w2, b2)
    g = np.random.default_rng(100 + seed)
    for _ in range(8):
        h = np.maximum(g.normal(size=64), 0.0)                  # the operand is a ReLU output
        want, rstd = _reference_kv(W, b, gamma, beta, w2, b2, h)
        assert np.abs(rstd * (M @ h + c) + (W @ beta + b) - want).max() <= 1e-12
        w2c, b2c = w2 - w2.mean(axis=0, keepdims=True), b2 - b2.mean()
        assert np.abs((M @ h + c) - (W * gamma) @ (w2c @ h + b2c)).max() <= 1e-12


def test_fold_is_the_layer_behind_the_layernorm_at_trained_weights():
    g = np.random.default_rng(7)
    seen = 0
    for block, (W, b, gamma, beta, w2, b2) in _trained_cases():
        assert np.abs(b2).max() > 0.05 and np.abs(gamma - 1).max() > 0.1, block      # the profile moved what the fold folds
        M, c = T.composite(W, gamma, w2, b2)
        assert np.abs(c).max() > 1e-3, block                    # ... so the constant the kernel starts from is not zero
        for _ in range(4):
            h = np.maximum(g.normal(size=64), 0.0)
            want, rstd = _reference_kv(W, b, gamma, beta, w2, b2, h)
            assert np.abs(rstd * (M @ h + c) + (W @ beta + b) - want).max() <= 1e-12, block
            w2c, b2c = w2 - w2.mean(axis=0, keepdims=True), b2 - b2.mean()
            assert np.abs((M @ h + c) - (W * gamma) @ (w2c @ h + b2c)).max() <= 1e-12, block
        seen += 1
    assert seen == 4                                            # lin_k and lin_v of both blocks


def test_image_read_from_the_consumers_side_is_the_composite():
    """the twin's fragment image, read back by the rule the matrix-core product reads it (tile.hpp), is the composite to the 22 bits
    of two fp16 pieces (the fp32 rounding included); and a host re-pack reproduces it word for word"""
    W, _, gamma, _, w2, b2 = _random_case(5)
    M, c = T.composite(W, gamma, w2, b2)
    img = T.fragment_image(M)
    back = T.matrix_of_image(img)
    assert np.abs(back - M).max() <= 2.0 ** -21 * np.abs(M).max()
    hi, lo = T.split_fp16(M.astype(np.float32))
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), back)
    # element (row 16 jo + i, feature 32 s + 16 (j >> 2) + 4 g + (j & 3)) sits at [jo][s][piece][16 g + i][j]: spot checks from the formula
    for jo, s, lane, j in ((0, 0, 0, 0), (3, 1, 63, 7), (2, 0, 37, 5), (1, 1, 16, 2)):
        row, feat = 16 * jo + (lane & 15), 32 * s + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
        assert img[jo, s, 0, lane, j] == hi[row, feat].view(np.uint16) and img[jo, s, 1, lane, j] == lo[row, feat].view(np.uint16)
    words = T.fold_image(W, 2 * W, gamma, w2, b2)
    assert words.dtype == np.float32 and words.size == 8320
    assert np.array_equal(words[:4096].view(np.uint16), img.reshape(-1))
    assert np.array_equal(words[4096:8192].view(np.uint16), T.fragment_image(2 * M).reshape(-1))     # lin_v's half follows lin_k's
    assert np.array_equal(words[8192:8256], c.astype(np.float32)) and np.array_equal(words[8256:], (2 * c).astype(np.float32))


def test_binding_of_the_image_offsets_matches_the_layout_header():
    """_lib.EDGE_FUSED_IMAGE_FLOATS / EDGE_FOLD_IMAGE_FLOATS against the fields of EdgeL6F in csrc/layouts.hpp, summed here"""
    import os
    from trajsde_amd import _lib
    text = open(os.path.join(H.ROOT, "trajsde_amd", "csrc", "layouts.hpp")).read()
    body = re.search(r"struct EdgeL6F \{(.*?)\n\};", text, flags=re.S).group(1)
    consts = {"MAT64X6": 4096, "In2L::SIZE": 200, "IN2F": 1024}
    sizes = {}
    for name, size, _prev in re.findall(r"TS_FIELD\((\w+), ([^,]+), (\w+)\)", body):
        for k, v in consts.items():
            size = size.replace(k, str(v))
        sizes[name] = int(eval(size, {"__builtins__": {}}))
    order = list(sizes)
    assert order[-2:] == ["MKV", "CKV0"] and order[-4:-2] == ["CK", "CV"]
    assert sum(sizes.values()) == _lib.EDGE_FUSED_IMAGE_FLOATS
    assert sizes["MKV"] + sizes["CKV0"] == _lib.EDGE_FOLD_IMAGE_FLOATS == 2 * 4096 + 128
    assert sizes["MKV"] == sizes["WKV"]                          # the composite takes the plain image's slot in LDS
    off = _lib.edge_fold_offsets(1_000_000)
    assert off["al"] + _lib.EDGE_FOLD_IMAGE_FLOATS == 1_000_000 and off["al"] - off["aa"] == _lib.EDGE_FUSED_IMAGE_FLOATS
    lib = _lib.lib()
    if lib.trajsde_split_products() == 3:                       # the fp16x3 build: the encoder blob holds both images
        assert lib.trajsde_blob_floats(_lib.STAGE_ENCODER, 0, 0) > 2 * _lib.EDGE_FUSED_IMAGE_FLOATS
