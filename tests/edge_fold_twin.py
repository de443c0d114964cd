"""numpy float64 twin of the folded key / value image of the fused edge attention (csrc/pack.hip PK_MAT6_FOLD / PK_VEC_FOLD,
csrc/layouts.hpp EdgeL6F MKV | CKV0), for tests/test_edge_fold_cpu.py and tests/test_gpu_edge_fold.py.

The last LayerNorm of MultipleInputEmbedding is  LN(y) = gamma (y - mean y) rstd + beta  on  y = W2 h' + b2.  With the feature-centred
W2c = W2 - 1 (1^T W2) / 64 and b2c = b2 - mean(b2),  y - mean y = W2c h' + b2c, and for W one of lin_k / lin_v

    W LN(y) + b  =  rstd (M h' + c) + (W beta + b)      M = W diag(gamma) W2c,   c = W diag(gamma) b2c.

The kernel multiplies by M (as two fp16 pieces per element, in matrix-core fragment order), starts from c and applies rstd last."""
import numpy as np


def composite(W, gamma, w2, b2):
    """(M [64, 64], c [64]) in float64 from the raw parameters"""
    W, gamma, w2, b2 = (np.asarray(a, dtype=np.float64) for a in (W, gamma, w2, b2))
    w2c = w2 - w2.mean(axis=0, keepdims=True)
    b2c = b2 - b2.mean()
    return (W * gamma[None, :]) @ w2c, (W * gamma[None, :]) @ b2c


def split_fp16(x32):
    """the two fp16 pieces of an fp32 array as pack.hip store_split forms them: hi = fp16(x) and lo = fp16(x - hi), round to nearest"""
    x32 = np.asarray(x32, dtype=np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def fragment_image(M):
    """uint16 image [jo 0..3][s 0..1][piece 0..1][lane 0..63][j 0..7] of a 64 x 64 matrix: element j of lane (i, g) in k-step s is the
    piece of M[16 jo + i][32 s + 16 (j >> 2) + 4 g + (j & 3)]  (csrc/pack.hip k_pack_mat6)"""
    hi, lo = split_fp16(np.asarray(M, dtype=np.float64).astype(np.float32))
    img = np.zeros((4, 2, 2, 64, 8), dtype=np.uint16)
    lane = np.arange(64)
    i, g = lane & 15, lane >> 4
    for jo in range(4):
        for s in range(2):
            for j in range(8):
                col = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3)
                img[jo, s, 0, :, j] = hi[16 * jo + i, col].view(np.uint16)
                img[jo, s, 1, :, j] = lo[16 * jo + i, col].view(np.uint16)
    return img


def matrix_of_image(img):
    """the float64 matrix hi + lo that a kernel reading `img` (uint16, fragment_image's shape or flat) multiplies by -- written from
    the READER's side (csrc/tile.hpp: lane (n, g) supplies, in slot j of k-step s, feature 32 s + 16 (j >> 2) + 4 g + (j & 3), and the
    fragment of lane (i, g) holds row 16 jo + i at that feature)"""
    img = np.asarray(img, dtype=np.uint16).reshape(4, 2, 2, 64, 8)
    M = np.zeros((64, 64), dtype=np.float64)
    for jo in range(4):
        for s in range(2):
            for lane in range(64):
                for j in range(8):
                    row, feat = 16 * jo + (lane & 15), 32 * s + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
                    M[row, feat] = float(img[jo, s, 0, lane, j:j + 1].view(np.float16)[0]) + float(img[jo, s, 1, lane, j:j + 1].view(np.float16)[0])
    return M


def fold_image(wk, wv, gamma, w2, b2):
    """the MKV | CKV0 image as float32 words (8320 of them): the lin_k composite's fragment image, the lin_v composite's, c_k, c_v"""
    mk, ck = composite(wk, gamma, w2, b2)
    mv, cv = composite(wv, gamma, w2, b2)
    words = [fragment_image(m).reshape(-1).view(np.float32) for m in (mk, mv)]
    return np.concatenate(words + [ck.astype(np.float32), cv.astype(np.float32)])


def block_parameters(sd, block):
    """(wk, wv, gamma3, w2, b2) of `block` "aa" or "al" from a model's state dict, as float64 arrays"""
    att, emb = {"aa": ("encoder.aa_encoder", "encoder.aa_encoder.nbr_embed"), "al": ("encoder.al_encoder", "encoder.al_encoder.lane_embed")}[block]
    names = (att + ".lin_k.weight", att + ".lin_v.weight", emb + ".aggr_embed.3.weight", emb + ".aggr_embed.2.weight", emb + ".aggr_embed.2.bias")
    return tuple(sd[n].detach().cpu().double().numpy() for n in names)
