"""Monte-Carlo decoding (include/trajsde_hip_mc.h, runtime.StageRuntime.decoder_forward_mc, PredictionModelSDENet.predict_samples),
the parts that need no GPU: the extension header against `_lib.MC_EXT_SIGNATURES`, the exported symbols, the refusals of the host side of
the entry point and of the Python surface, the float64 twin of the device reduction (runtime.mc_statistics_host) against numpy, the
kernels' resource listing, and the driver's switch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers as H

NAMES = {"trajsde_decoder_mc_ws_bytes", "trajsde_decoder_forward_mc"}
K, T = 3, 5


def test_mc_header_and_its_signature_table_agree(tmp_path):
    """include/trajsde_hip_mc.h against `_lib.MC_EXT_SIGNATURES`, by the rules tests/test_capacity_cpu.py applies to its header"""
    import test_cabi_cpu as CABI
    from trajsde_amd import _lib
    inc = os.path.join(H.ROOT, "include")
    text = open(os.path.join(inc, "trajsde_hip_mc.h")).read()
    assert '#include "trajsde_hip.h"' in text
    body = text.replace('#include "trajsde_hip.h"', "")
    declared = set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)))
    assert declared == set(_lib.MC_EXT_SIGNATURES) == NAMES
    for other in (_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.COT_SEL_EXT_SIGNATURES, _lib.GRID_EXT_SIGNATURES, _lib.CLIP_EXT_SIGNATURES,
                  _lib.ENC_COT_EXT_SIGNATURES, _lib.CAPACITY_EXT_SIGNATURES):
        assert not set(_lib.MC_EXT_SIGNATURES) & set(other)
    for h in sorted(os.listdir(inc)):
        if h != "trajsde_hip_mc.h":
            assert not declared & set(re.findall(r"\b(trajsde_[a-z_0-9]+)\s*\(", open(os.path.join(inc, h)).read())), h
    protos = CABI._header_prototypes(body)
    assert set(protos) == declared
    assert CABI._check_against_header(_lib.MC_EXT_SIGNATURES, protos) == []
    swap = lambda tu: tu.replace('#include "trajsde_hip.h"', '#include "trajsde_hip_mc.h"')
    r = CABI._compile_tu(swap(CABI._prototype_tu(_lib.MC_EXT_SIGNATURES, protos)), tmp_path, H.ROOT, "mc")
    assert r.returncode == 0, r.stdout[-3000:]
    for name in NAMES:                                          # the check has teeth: one argument fewer is caught both ways
        bad = dict(_lib.MC_EXT_SIGNATURES)
        res, args = bad[name]
        bad[name] = (res, args[:-1])
        assert CABI._check_against_header(bad, protos)
        assert CABI._compile_tu(swap(CABI._prototype_tu(bad, protos)), tmp_path, H.ROOT, "mc_bad").returncode != 0
    assert _lib.ABI_VERSION == 10 and _lib.lib().trajsde_abi_version() == 10   # an extension header: the ABI version did not move
    assert int(re.search(r"#define TRAJSDE_MC_MAX_SAMPLES (\d+)", text).group(1)) == _lib.MC_MAX_SAMPLES


def test_both_symbols_are_exported_by_the_built_library():
    from trajsde_amd import _lib
    lib = _lib.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.MC_EXT_SIGNATURES[name][1]
    assert lib.trajsde_abi_version() == 10


def test_entry_point_refuses_before_any_launch():
    """null pointers, n_samples < 2, a stride that overflows the 32-bit counter row, a short workspace: refused on the host with the
    reason in trajsde_last_error; the stand-in addresses are never dereferenced"""
    from trajsde_amd import _lib
    L = _lib.lib()
    p = 0x7E0000000000
    N = 14
    noise = _lib.Noise(C.c_uint64(1), None, None, None)
    need = L.trajsde_decoder_mc_ws_bytes(N, K, T, 17)
    # y0 [K N, 64] fp32 + two tiles of 8-float partials per (path, step), each rounded up to 256 bytes, + 256
    assert need == (K * N * 64 * 4 + 255) // 256 * 256 + (2 * K * N * T * 8 * 4 + 255) // 256 * 256 + 256
    assert L.trajsde_decoder_mc_ws_bytes(N, K, T, 16) < need < L.trajsde_decoder_mc_ws_bytes(N, K, T, 33)

    def call(R=17, D=K * N, ws=p, ws_bytes=need, blob=p, loc_mean=p, loc_cov=p, pi=p, milstein=0):
        rc = L.trajsde_decoder_forward_mc(N, K, T, milstein, blob, p, p, p, 6, p, 0.1, C.byref(noise), R, D, ws, ws_bytes, loc_mean, loc_cov,
                                          None, None, pi, None)
        return rc, (L.trajsde_last_error() or b"").decode()

    for kw in (dict(blob=None), dict(loc_mean=None), dict(loc_cov=None), dict(pi=None), dict(ws=None)):
        assert call(**kw) == (-1, "decoder_forward_mc: null pointer"), kw
    for R in (1, 0, -3):
        rc, msg = call(R=R)
        assert rc == -1 and "n_samples must be at least 2" in msg
    assert call(R=_lib.MC_MAX_SAMPLES + 1)[0] == -1
    for R, D in ((2, 0), (2, -1), (2, 2 ** 32 - K * N + 1), (17, (2 ** 32 - K * N) // 16 + 1), (2, 2 ** 40)):
        rc, msg = call(R=R, D=D)
        assert rc == -1 and "sample_stride" in msg, (R, D, msg)
    rc, msg = call(ws_bytes=need - 1)
    assert rc == -3 and "workspace too small" in msg
    for args in ((0, K, T, 17), (N, 0, T, 17), (N, K, 0, 17), (N, K, T, 1), (N, K, T, _lib.MC_MAX_SAMPLES + 1)):
        assert L.trajsde_decoder_mc_ws_bytes(*args) == -1 and b"decoder_mc_ws_bytes" in L.trajsde_last_error()
    # the largest admitted stride passes the argument checks (what stops the call on a host without a GPU is the first launch)
    rc, msg = call(R=2, D=2 ** 32 - K * N)
    assert not (rc == -1 and "sample_stride" in msg), msg


@pytest.mark.parametrize("R", [2, 3, 17, 33])
def test_mc_statistics_host_matches_numpy(R):
    from trajsde_amd.runtime import mc_statistics_host
    rng = np.random.default_rng(R)
    x = (rng.standard_normal((R, 3, 7, 5, 4)) * np.array([0.7, 0.3, 0.1, 0.1]) + np.array([1000.0, -1000.0, 1.0, 2.0])).astype(np.float32)
    mean, cov = mc_statistics_host(torch.from_numpy(x))
    assert mean.dtype == cov.dtype == torch.float64 and tuple(mean.shape) == (3, 7, 5, 4) and tuple(cov.shape) == (3, 7, 5, 3)
    x64 = x.astype(np.float64)
    assert np.abs(mean.numpy() - x64.mean(axis=0)).max() < 1e-12
    want = np.empty((3, 7, 5, 3))
    flat = x64.reshape(R, -1, 4)
    for i in range(flat.shape[1]):
        c = np.cov(flat[:, i, 0], flat[:, i, 1], ddof=1)
        want.reshape(-1, 3)[i] = (c[0, 0], c[1, 1], c[0, 1])
    assert np.abs(cov.numpy() - want).max() < 1e-12
    assert float(cov[..., :2].min()) > 0.0
    mean2, cov2 = mc_statistics_host(torch.from_numpy(x[..., :2]))           # `uncertain: False` samples: two channels
    assert torch.equal(mean2, mean[..., :2]) and torch.equal(cov2, cov)


def test_mc_statistics_host_refuses_one_sample():
    from trajsde_amd import _lib
    from trajsde_amd.runtime import mc_statistics_host
    with pytest.raises(_lib.TrajsdeError, match="R >= 2"):
        mc_statistics_host(torch.zeros(1, 3, 4))
    with pytest.raises(_lib.TrajsdeError):
        mc_statistics_host(torch.zeros(4, 3, 1))


def test_python_surface_refuses_before_the_gpu():
    """n_samples < 2, an overflowing stride, tensors on the host (no CPU implementation), train mode"""
    from trajsde_amd import _lib
    from trajsde_amd.runtime import NoiseSpec, mc_check_arguments
    from trajsde_amd.synth import synth
    batch = synth(S=2, n=7, L=4, F=T, box=60.0, seed=5)
    N = batch.num_nodes
    model, cfg = H.build_model(K, T, 0.5, init_seed=7)
    assert mc_check_arguments(17, K * N) == (17, K * N) and mc_check_arguments(2, K * N, 2 ** 32 - K * N) == (2, 2 ** 32 - K * N)
    local, glob = torch.zeros(N, 64), torch.zeros(K, N, 64)
    for R in (1, 0, -2, 2.5):
        with pytest.raises(_lib.TrajsdeError, match="n_samples"):
            model.predict_samples(H.clone_batch(batch), R)
        with pytest.raises(_lib.TrajsdeError, match="n_samples"):
            model.decoder.sample(batch, local, glob, R)
    with pytest.raises(_lib.TrajsdeError, match="n_samples"):
        model.predict_samples(H.clone_batch(batch), _lib.MC_MAX_SAMPLES + 1)
    for R, D in ((2, 0), (2, 2 ** 32 - K * N + 1), (17, 2 ** 28), (3, -5)):
        with pytest.raises(_lib.TrajsdeError, match="sample_stride"):
            model.predict_samples(H.clone_batch(batch), R, sample_stride=D)
        with pytest.raises(_lib.TrajsdeError, match="sample_stride"):
            model.decoder._rt.decoder_forward_mc(batch, local, glob, R, sample_stride=D)
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        model.predict_samples(H.clone_batch(batch), 4, noise=NoiseSpec(seed=1))
    with pytest.raises(_lib.TrajsdeError, match="must live on the GPU"):
        model.decoder.sample(batch, local, glob, 4, noise=NoiseSpec(seed=1))
    model.train()
    try:
        with pytest.raises(_lib.TrajsdeError, match="inference only"):
            model.predict_samples(H.clone_batch(batch), 4)
        with pytest.raises(_lib.TrajsdeError, match="inference only"):
            model.decoder.sample(batch, local, glob, 4)
    finally:
        model.eval()


def test_driver_knows_mc_samples():
    import inspect
    from trajsde_amd import driver
    ap = driver.arg_parser()
    assert ap.parse_args(["-c", "x.yml"]).mc_samples is None
    assert ap.parse_args(["-c", "x.yml", "--mc-samples", "16"]).mc_samples == 16
    assert ap.parse_args(["-c", "x.yml", "--mc_samples", "4"]).mc_samples == 4
    assert inspect.signature(driver.evaluate).parameters["mc_samples"].default is None
    from trajsde_amd.models.model_base_mix import PredictionModel
    assert not hasattr(PredictionModel, "predict_samples")      # the vanilla variant's decoder is deterministic
    with pytest.raises(ValueError, match="deterministic"):
        driver.evaluate(object(), [], mc_samples=4)


@pytest.mark.parametrize("extra,expect", [([], 8), (["-DTSDE_SPLIT_H3=0"], 3)])
def test_mc_decode_kernels_compile_without_scratch(tmp_path, extra, expect):
    """every instantiation of k_sde_decode_mc holds its state, the sample bookkeeping and the reduction in registers (fp16x3: Euler and
    Milstein, split and plain image, 512 and 768 threads; bf16x6: the 512-thread builds only -- its 768-thread builds spill, like
    k_sde_decode's); the reduction is cross-lane register traffic (DPP), and the unit carries none of the vectoriser's register-pair moves"""
    from trajsde_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    out = tmp_path / "decoder_mc.s"
    src = os.path.join(H.ROOT, "trajsde_amd", "csrc", "decoder_mc.hip")
    subprocess.check_call([build.HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-o", str(out), src], stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN4tsde15k_sde_decode_mcILb[01]ELi\d+ELb[01]E\w+):.*?; ScratchSize: (\d+)", text, flags=re.S | re.M)
    assert len(kernels) == expect, kernels
    assert all(int(sz) == 0 for _, sz in kernels), kernels
    assert len(re.findall(r"^_ZN4tsde12k_mc_combine\w+:", text, flags=re.M)) == 1
    assert "row_mirror" in text and "quad_perm" in text and "v_pk_mov_b32" not in text
    atomics = set(re.findall(r"^\s+(\w*atomic\w*)", text, flags=re.M))     # the range guard's sticky bit is the unit's only atomic
    assert atomics <= {"global_atomic_or"}, atomics
