"""Host-side runtime of the stage modules: weight packing, workspaces, noise selection and the ctypes
calls into libtrajsde_hip.so.  PyTorch is used for device memory and streams only."""
import collections.abc
import ctypes as C
import itertools
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from trajsde_amd import _lib
from trajsde_amd.schedule import EulerSchedule, decoder_schedule, encoder_schedule

D = 64


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.TrajsdeError(f"{what} must live on the GPU: the hot path has no CPU implementation "
                                "(oracle/ is test infrastructure, not a fallback)")


@dataclass
class NoiseSpec:
    """Where the path's randomness comes from (SURVEY.md App. F draw order).

    seed            in-kernel Philox4x32-7 key; host twin: trajsde_amd/philox.py
    z_fake/z_enc/z_dec   injected standard normals [A,21,2] / [21,Nt,64] / [n_euler,K*N,64] (parity tests)
    *_row_ids       int32 global row ids for the Philox counter (resharding-invariant streams)
    """
    seed: int = 0
    seed_dev: Optional[torch.Tensor] = None  # one uint64 (as int64) on the device: the key is read THERE when the kernels run
                                             # (`seed` ignored) -- what lets a captured graph of the forward draw fresh noise
    dropout_seed: Optional[int] = None       # key of the train-mode dropout masks (csrc/dropout.hpp); default: `seed`
    z_fake: Optional[torch.Tensor] = None
    z_enc: Optional[torch.Tensor] = None
    z_dec: Optional[torch.Tensor] = None
    fake_row_ids: Optional[torch.Tensor] = None
    enc_row_ids: Optional[torch.Tensor] = None
    dec_row_ids: Optional[torch.Tensor] = None

    @staticmethod
    def resolve(noise: Optional["NoiseSpec"]) -> "NoiseSpec":
        if noise is not None:
            return noise
        return NoiseSpec(seed=int(torch.randint(0, 2 ** 62, (1,)).item()))   # fresh stream per forward, like the reference

    def c_dropout(self, module) -> Optional[_lib.Dropout]:
        """the stage's `dropout` kwarg as the C struct while the module is in train mode, else None (eval: no dropout)"""
        p = float(getattr(module, "dropout", 0.0) or 0.0)
        if not getattr(module, "training", False) or p <= 0.0:
            return None
        if self.dropout_seed is None and self.seed_dev is not None:
            raise _lib.TrajsdeError("train-mode dropout with a device-resident Philox key (seed_dev): the mask key is a host "
                                    "value -- pass NoiseSpec(dropout_seed=...)")
        ds = self.seed if self.dropout_seed is None else self.dropout_seed
        return _lib.Dropout(C.c_float(p), C.c_uint64(int(ds) & 0xFFFFFFFFFFFFFFFF))

    def c_noise(self, z: Optional[torch.Tensor], row_ids: Optional[torch.Tensor]) -> _lib.Noise:
        if z is not None:
            assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous()
        if row_ids is not None:
            assert row_ids.is_cuda and row_ids.dtype == torch.int32 and row_ids.is_contiguous()
        if self.seed_dev is not None:
            assert self.seed_dev.is_cuda and self.seed_dev.dtype == torch.int64 and self.seed_dev.numel() == 1
        return _lib.Noise(C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), _ptr(z), _ptr(row_ids), _ptr(self.seed_dev))


class GraphedForward:
    """The inference forward of one batch captured in a HIP graph (torch.cuda.CUDAGraph) and replayed.

    Possible because the forward is sync-free (trajsde_graph_prepare_async: list lengths stay on the device, buffers and grids are
    sized from bounds) and the Philox key can live in device memory (NoiseSpec.seed_dev): a replay re-runs graph preparation,
    encoder, global interactor and decoder on whatever the batch tensors hold NOW, with the key written before the replay.
    The batch tensors must keep their shapes and addresses (update them in place); outputs are the captured tensors.
    `model`: the SDE model, also with `model.ood = True` (the key seeds the `n_samples` recurrences, the outputs include `stds`).
    The vanilla HiVT PredictionModel is refused: its forward is sync-free and was captured and replayed bit for bit at small shapes,
    but ten back-to-back replays at 64 x 128 agents ended in the look-back guard of the graph stage's prefix sum (prep.hip
    lookback_prefix: a predecessor's word read as never published) and the cause is not found -- DESIGN.md section 7.

        gf = GraphedForward(model, batch)          # warm-up + capture
        out = gf(seed=123)                         # one graph launch; out["loc"] etc. are overwritten by the next call
    """

    def __init__(self, model, data, warmup: int = 2) -> None:
        x = data["x"]
        _require_gpu(x, "data['x']")
        if not sync_free():
            raise _lib.TrajsdeError("GraphedForward needs the sync-free forward (TRAJSDE_SYNC_FREE, default kernel forms)")
        if model.training:
            raise _lib.TrajsdeError("GraphedForward captures the inference forward: call model.eval() first")
        enc_rt = getattr(getattr(model, "encoder", None), "_rt", None)
        if enc_rt is not None and enc_rt.stage == "encoder_grid":
            raise _lib.TrajsdeError("GraphedForward does not capture the vanilla HiVT model: replays of its graph at 64 x 128 agents ended "
                                    "in the graph stage's look-back guard and the cause is not found (DESIGN.md section 7); its eager "
                                    "forward is sync-free")
        self.model, self.data = model, data
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=x.device)
        self.noise = NoiseSpec(seed=0, seed_dev=self.seed_dev)
        self._y = data.y                                                    # the forward REBINDS data.y to the rotated copy (MODEL:83-84):
        side = torch.cuda.Stream(device=x.device)                          # the captured kernels keep reading this tensor
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):                                  # weight images packed, LDS limits raised, pools warm
                data.y = self._y
                model(data, noise=self.noise)
        torch.cuda.current_stream(x.device).wait_stream(side)
        torch.cuda.synchronize(x.device)
        for mod in model.modules():                                          # every weight image is packed and the device is idle:
            rt = getattr(mod, "_rt", None)                                   # drop the pack-done events, so that blob() does not
            if isinstance(rt, StageRuntime):                                 # query one inside the capture (not capturable)
                rt.packs_complete()
        if GraphContext.KEY in data:                                         # the capture must contain the graph stage itself
            del data[GraphContext.KEY]
        self.graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(device=x.device)                             # the capture stream and its side stream (the relative-pose
        _side_stream(x.device, cap)                                          # prefetch forks onto it) exist before the capture starts
        with torch.cuda.graph(self.graph, stream=cap), torch.no_grad():
            data.y = self._y
            self.out = model(data, noise=self.noise)
        if GraphContext.KEY in data:                                         # its lists live in the capture's pool and hold nothing before the
            del data[GraphContext.KEY]                                       # first replay: an eager forward of this batch builds its own

    def __call__(self, seed: int):
        self.seed_dev.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        self.graph.replay()
        return self.out


def set_state_storage(kind: str) -> str:
    """"fp32" (default) or "bf16": how the [rows][64] activations that stay inside a stage are stored between its kernels
    (include/trajsde_hip.h trajsde_state_storage; BASELINE configs[4] "bf16 hidden state").  Inference only.  Returns the
    previous setting."""
    if kind not in ("fp32", "bf16"):
        raise ValueError("state storage is 'fp32' or 'bf16'")
    return "bf16" if _lib.lib().trajsde_state_storage(1 if kind == "bf16" else 0) else "fp32"


# Off by default: measured on the metric workload (32 x 256 agents) the one-stream forward gains 0.6 % (2.781 against 2.798 ms)
# and the three-stream headline loses 1.2 % -- the recurrence's four waves per CU hold the whole register file of their SIMDs
# (512 registers each), so the embedding kernel only finds room on the CUs the recurrence leaves empty (HISTORY.md section 5).
_OVERLAP_REL = os.environ.get("TRAJSDE_OVERLAP_REL", "0") != "0"
_SIDE_STREAMS: Dict[tuple, "torch.cuda.Stream"] = {}


def _side_stream(dev, cur) -> "torch.cuda.Stream":
    """one side stream per (device, stream the forward runs on): forwards dealt over several streams keep their own"""
    key = (str(dev), int(cur.cuda_stream))
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


class RelPrefetch:
    """the aggregator's relative-pose rows on their way on a side stream (StageRuntime.prefetch_rel_embed)"""

    def __init__(self, gc, ws, ws_bytes, done, dev) -> None:
        self.gc, self.ws, self.ws_bytes, self.done, self.dev = gc, ws, ws_bytes, done, dev
        self.joined = False

    def join(self) -> None:
        """the current stream waits for the side stream's kernel (also what ends a captured fork)"""
        if not self.joined:
            torch.cuda.current_stream(self.dev).wait_event(self.done)
            self.joined = True


_SYNC_FREE = os.environ.get("TRAJSDE_SYNC_FREE", "1") != "0"
SYNC_FREE_MAX_BYTES = 4 << 30
# ... and for the training loop's prefetched graphs: TWO batches are alive at once there and the bound-sized lists keep their size
# after make_exact() (at 32 x 256 agents ~2 GB a batch where the exact build needs ~160 MB), so the prefetch path gets half the cap
# -- at most 2 x 2 GB of the 288 GB reserved by it (the shipped training shapes need 0.3-1.0 GB) -- and beyond it takes the
# synchronising form: its one host read then waits on the side stream, which is what the form was before round 5
PREFETCH_SYNC_FREE_MAX_BYTES = 2 << 30


def set_sync_free(on: bool) -> bool:
    """Sync-free inference forward (default on): the graph stage leaves the compacted lists' lengths on the device
    (trajsde_graph_prepare_async) and sizes buffers and grids from bounds, so a forward never waits on the GPU.  Entry points
    that need the lengths on the host (training, backward, captures) make the graph exact themselves.  Returns the previous
    setting."""
    global _SYNC_FREE
    prev, _SYNC_FREE = _SYNC_FREE, bool(on)
    return prev


def sync_free() -> bool:
    return _SYNC_FREE and bool(_lib.lib().trajsde_sync_free_supported())


def state_storage() -> str:
    L = _lib.lib()
    prev = L.trajsde_state_storage(0)
    L.trajsde_state_storage(prev)
    return "bf16" if prev else "fp32"


def rotate_inputs(data) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """MODEL:75-85 on the GPU: rotate_mat [N,2,2] and y @ rotate_mat."""
    ang = data["rotate_angles"]
    _require_gpu(ang, "data['rotate_angles']")
    N = ang.shape[0]
    y = data.y
    rot = torch.empty(N, 2, 2, device=ang.device, dtype=torch.float32)
    y_rot = torch.empty_like(y) if y is not None else None
    F = y.shape[1] if y is not None else 0
    _lib.check(_lib.lib().trajsde_rotate(_ptr(ang.contiguous()), N, _ptr(y.contiguous()) if y is not None else None, F,
                                         _ptr(rot), _ptr(y_rot), _stream()), "trajsde_rotate")
    return rot, y_rot


ROTATED_KEY = "_trajsde_rotated"          # set by prefetch_graph: MODEL:76-85 has been applied to this batch already, once
_PREFETCH_STREAMS: Dict[str, "torch.cuda.Stream"] = {}


def side_stream(device) -> "torch.cuda.Stream":
    """the stream next batches are prepared on while the current step runs (one per device)"""
    key = str(device)
    if key not in _PREFETCH_STREAMS:
        _PREFETCH_STREAMS[key] = torch.cuda.Stream(device=device)
    return _PREFETCH_STREAMS[key]


_COLLECTIVE_STREAMS: Dict[str, "torch.cuda.Stream"] = {}


def collective_stream(device) -> "torch.cuda.Stream":
    """the stream the early slice of the gradient all-reduce runs on (driver.FlatGrads.early_reduce), one per device and NOT the
    prefetch stream: the collective must neither queue behind the next batch's graph stage nor hold that stage back"""
    key = str(device)
    if key not in _COLLECTIVE_STREAMS:
        _COLLECTIVE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _COLLECTIVE_STREAMS[key]


def prefetch_graph(data, radius: float, H: int, noise: "NoiseSpec", fake_agents: bool = True, main_stream=None) -> None:
    """Rotation (MODEL:76-85) and graph stage of a batch the training loop will use NEXT, on the side stream -- call it under
    `torch.cuda.stream(side_stream(dev))`, with the batch's tensors produced on that stream as well (driver.train moves the next
    batch to the device there).  The graph stage holds the one host synchronisation of a training step (the list lengths size the
    tapes): taken here it waits for a few small kernels on the side stream while the main stream still holds milliseconds of the
    current step, and the next `training_step` starts enqueueing at once -- taken inside the step the GPU idles from the last
    optimizer kernel until the host has woken up and launched again.  Everything made here is handed to the main stream (event +
    allocator bookkeeping); `training_step` finds the rotation marked done and the graph cached on the batch."""
    dev = data["x"].device
    side = torch.cuda.current_stream(dev)
    main = main_stream if main_stream is not None else torch.cuda.default_stream(dev)      # the stream the training step runs on
    if side == main:
        raise _lib.TrajsdeError("prefetch_graph must run under torch.cuda.stream(runtime.side_stream(device))")
    rot, y_rot = rotate_inputs(data)
    if y_rot is not None:
        data.y = y_rot
    data["rotate_mat"] = rot
    data[ROTATED_KEY] = True
    # The list lengths (the step's one host read-back) are NOT waited for here: the graph is built in its sync-free form -- lengths on
    # the device, lists sized by their bounds -- and made exact at the top of the step that uses it, by a read issued on THIS stream
    # (GraphContext.make_exact honours `count_stream`), which by then has long drained.  Waiting here cost the loop 0.3-0.7 ms a
    # step: the side stream's few kernels share the chip with the step that was just enqueued.  Lists past
    # PREFETCH_SYNC_FREE_MAX_BYTES (two batches are alive in this loop, and bound-sized lists keep their size) take the synchronising form.
    gc = GraphContext.get(data, radius, H, noise, fake_agents=fake_agents, exact=not sync_free(), sync_free_cap=PREFETCH_SYNC_FREE_MAX_BYTES)
    gc.count_stream = side
    done = torch.cuda.Event()
    done.record(side)
    main.wait_event(done)
    for t in _tensors_in(list(data.as_dict().values()) + [gc.ws, gc.edges_ws, gc.rot] + list(gc._keep)):
        if t.is_cuda:
            t.record_stream(main)                       # freed while main-stream kernels still read it: not handed out again before they finish


def _tensors_in(obj):
    """every tensor inside nested lists / tuples / dicts (batch fields may hold containers of tensors)"""
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors_in(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors_in(v)


def consume_rotation(data) -> bool:
    """True once for a batch that prefetch_graph has rotated already (the caller then skips MODEL:76-85)"""
    if ROTATED_KEY in data:
        del data[ROTATED_KEY]
        return True
    return False


def edge_snapshots(data, historical_steps: int) -> None:
    """The encoder's side effect on the batch (ENC:88-99, 107-110): `data['edge_index_{t}']` = the edges of the EXTENDED
    edge list (edge_index plus the in-edges of the target agents re-pointed at their fake copies, node ids N..N+A-1) whose
    two endpoints are valid at step t, in the order of the input list, and `data['edge_attr_{t}']` = pos[src,t] - pos[dst,t]
    (no radius filter: ENC:115 applies it only to the copies fed to the AA encoder).  The HIP path never materialises these
    21 lists (it works on one target-sorted, radius-filtered list); stages write them only when asked to
    (`preserve_side_effects=True`), with plain device-side tensor indexing -- they feed nothing on the hot path."""
    ei, pad, pos, agent = data["edge_index"], data["padding_mask"], data["positions"], data["agent_index"]
    N = data["x"].shape[0]
    to_agent = torch.isin(ei[1], agent)
    _, inv = torch.unique(ei[1][to_agent], return_inverse=True)
    new_edge = torch.cat((ei, torch.stack((ei[0][to_agent], inv + N))), dim=-1)
    orig = torch.cat((torch.arange(N, device=ei.device), agent))
    valid, pos_ext = ~pad[orig][:, :historical_steps], pos[orig]
    for t in range(historical_steps):
        keep = valid[new_edge[0], t] & valid[new_edge[1], t]
        e = new_edge[:, keep]
        data[f"edge_index_{t}"] = e
        data[f"edge_attr_{t}"] = pos_ext[e[0], t] - pos_ext[e[1], t]


class _TableCache:
    """float32 schedule tables (host replay of the solver's time bookkeeping) resident on the device."""

    def __init__(self) -> None:
        self._c: Dict[tuple, tuple] = {}

    def get(self, key: tuple, make, device) -> Tuple[EulerSchedule, torch.Tensor, torch.Tensor]:
        k = key + (str(device),)
        if k not in self._c:
            s: EulerSchedule = make()
            self._c[k] = (s, torch.from_numpy(s.step_table()).to(device), torch.from_numpy(s.out_table()).to(device))
        return self._c[k]


_TABLES = _TableCache()
_ENC_TABLES: Dict[tuple, np.ndarray] = {}
_TABLES_DEV: Dict[tuple, torch.Tensor] = {}          # device copies of the host step tables



class GradLayout:
    """names / shapes / offsets of a *_BWD stage's gradient buffers inside their flat tensor -- static per stage"""

    def __init__(self, names, shapes) -> None:
        self.names, self.shapes = list(names), list(shapes)
        self.sizes = [int(np.prod(sh)) if len(sh) else 1 for sh in self.shapes]
        # 16-byte aligned slices: kernels store float4 rows into some of them
        self.offs, total = [], 0
        for sz in self.sizes:
            self.offs.append(total)
            total += (sz + 3) // 4 * 4
        self.total = total
        self.index = {n: i for i, n in enumerate(self.names)}
        self.byte_offs = np.asarray(self.offs, dtype=np.uint64) * np.uint64(4)


class GradBuffers(collections.abc.Mapping):
    """The zero-initialised gradient buffers of a *_BWD stage: ONE flat tensor (one fill instead of one per parameter), keyed and
    ordered like the stage's parameter names.  A read-only mapping name -> view; the views are made when they are asked for -- the
    training loop's sink (driver.FlatGrads.accumulate_bundles) adds the flat tensor into its own in one gather and never asks
    (creating ~250 views a step was 0.25 ms of host time, and walking them again in the sink as much)."""

    def __init__(self, flat: torch.Tensor, layout: GradLayout) -> None:
        self.flat, self.layout, self._views = flat, layout, {}

    def __getitem__(self, name: str) -> torch.Tensor:
        v = self._views.get(name)
        if v is None:
            lay = self.layout
            i = lay.index[name]
            v = self._views[name] = self.flat[lay.offs[i]:lay.offs[i] + lay.sizes[i]].view(lay.shapes[i])
        return v

    def __iter__(self):
        return iter(self.layout.names)

    def __len__(self) -> int:
        return len(self.layout.names)

    def __contains__(self, name) -> bool:
        return name in self.layout.index

    def pointer_array(self):
        """(ctypes pointer to the void* array the C-ABI takes, keep-alive object): base address + static byte offsets"""
        ptrs = self.layout.byte_offs + np.uint64(self.flat.data_ptr())
        return ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), ptrs


def single_call_forms() -> bool:
    """TRAJSDE_STEP_SINGLE_CALLS=0: a training step packs its weight images stage by stage, gathers its gradients and runs AdamW through
    torch's element-wise launches, as before ABI 10 (same results bit for bit: tests/test_gpu_step_launches.py) -- the A/B switch of
    profiles/r05_ab_runs.md"""
    return os.environ.get("TRAJSDE_STEP_SINGLE_CALLS", "1") != "0"


def _drop_scale_channels(module, out: dict) -> None:
    """`uncertain: False` (DEC:100-101, dec_hivt_nusargo_grid.py:58-59): 'loc' is [K, N, T, 2].  The kernels always evaluate both
    heads into [K, N, T, 4] (the absent scale head is a zero stand-in, params.ParamTree.absent); the four-channel tensor stays
    under a private key for the backward entry points, which index it"""
    if not getattr(module, "uncertain", True):
        out["_loc4"] = out["loc"]
        out["loc"] = out["loc"][..., :2].contiguous()


def _loc4(out: dict) -> torch.Tensor:
    loc = out.get("_loc4", out["loc"])
    if loc.shape[-1] != 4:
        raise _lib.TrajsdeError("the decoder backward needs the forward's own output dict (its [K, N, T, 4] locations)")
    return loc.contiguous()


def mc_check_arguments(n_samples, rows: int, sample_stride=None) -> Tuple[int, int]:
    """(R, D) of a Monte-Carlo decode over `rows` = K * N paths, or the refusal the entry point would give: R >= 2 (one sample is the
    plain forward), D >= 1 (default: `rows`) and (R - 1) * D + rows <= 2^32 -- the Philox counter row is 32 bits"""
    R = int(n_samples)
    if R != n_samples or R < 2:
        raise _lib.TrajsdeError(f"n_samples must be an integer >= 2, got {n_samples!r} (one sample is the plain forward)")
    if R > _lib.MC_MAX_SAMPLES:
        raise _lib.TrajsdeError(f"n_samples {R} is above {_lib.MC_MAX_SAMPLES}")
    stride = int(rows) if sample_stride is None else int(sample_stride)
    if stride < 1 or (R - 1) * stride + int(rows) > 2 ** 32:
        raise _lib.TrajsdeError(f"sample_stride {stride}: must be >= 1 with (n_samples - 1) * sample_stride + K * N <= 2^32 (sample s draws "
                                f"from Philox counter row id + s * sample_stride, a 32-bit word); got ({R} - 1) * {stride} + {int(rows)}")
    return R, stride


def mc_statistics_host(samples: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """the torch twin of the device reduction of decoder_forward_mc, in float64: `samples` [R, ..., C] (C >= 2: x, y, ...) ->
    (sample mean [..., C], unbiased sample covariance of (x, y) [..., 3]: var_x, var_y, cov_xy)"""
    if samples.dim() < 2 or samples.shape[0] < 2 or samples.shape[-1] < 2:
        raise _lib.TrajsdeError(f"samples must be [R >= 2, ..., C >= 2], got {tuple(samples.shape)}")
    x = samples.detach().to(torch.float64)
    mean = x.mean(dim=0)
    d = x[..., :2] - mean[..., :2]
    u = 1.0 / (x.shape[0] - 1)
    cov = torch.stack([(d[..., 0] ** 2).sum(0), (d[..., 1] ** 2).sum(0), (d[..., 0] * d[..., 1]).sum(0)], dim=-1) * u
    return mean, cov


class PackSet:
    """The weight images of several (StageRuntime, stage id) pairs packed by ONE call (trajsde_pack_weights_many: three launches
    over a job table that stays on the device).  A training step re-packs six images after every optimizer step -- 26 launches and 6
    fills of ~5 us through `StageRuntime.blob()` one stage at a time; `refresh()` at the top of the step leaves every `blob()` call
    of the step a cache hit.  The blobs are allocated once and re-packed in place: what reads them is ordered behind the pack on the
    packing stream, or behind its event on any other."""

    def __init__(self, entries) -> None:
        self.entries = list(entries)                 # [(StageRuntime, stage id)]
        self._blobs = None
        self._items = None
        self._tables = None                          # (pinned host table, device table, bytes)
        self._tab_ids = None
        self._fresh = 1

    def refresh(self) -> None:
        stamps = [rt._stamp() for rt, _ in self.entries]
        if self._blobs is not None:
            for (rt, sid), stamp, blob in zip(self.entries, stamps, self._blobs):
                cached = rt._blobs.get(sid)
                if cached is None or cached[1] != stamp or cached[0] is not blob:
                    break
            else:
                return                               # every image is current
        L = _lib.lib()
        first = self.entries[0][0]._first_param()
        _require_gpu(first, "parameters")
        dev = first.device
        tabs = [rt._param_table(sid) for rt, sid in self.entries]
        if self._blobs is None or any(b.device != dev for b in self._blobs):
            self._blobs = [torch.empty(t[3], device=dev, dtype=torch.float32) for t in tabs]
            self._items = None
        if self._items is None or any(a is not b for a, b in zip(self._tab_ids, tabs)):
            items = (_lib.PackItem * len(tabs))()
            for it, (rt, sid), t, blob in zip(items, self.entries, tabs, self._blobs):
                nl, K = rt._dims()
                it.stage, it.num_layers, it.num_modes, it.n_params = sid, nl, K, t[2]
                it.params = C.cast(t[1], C.c_void_p)
                it.blob, it.blob_floats = blob.data_ptr(), t[3]
            need = int(L.trajsde_pack_many_table_bytes(items, len(tabs)))
            if need < 0:
                raise _lib.TrajsdeError("trajsde_pack_many_table_bytes: unknown stage")
            if self._tables is None or self._tables[2] < need or self._tables[1].device != dev:
                self._tables = (torch.empty(need, dtype=torch.uint8).pin_memory(), torch.empty(need, dtype=torch.uint8, device=dev), need)
                self._fresh = 1
            self._items, self._tab_ids = items, tabs
        host, table, nbytes = self._tables
        with torch.cuda.device(dev):
            # the images are re-packed IN PLACE: streams that read them since the last pack (StageRuntime.blob records them) may still
            # have kernels queued on the old contents -- the pack waits for what they hold now
            packing = torch.cuda.current_stream()
            for (rt, sid), blob in zip(self.entries, self._blobs):
                for sid_, readers in list(rt._readers.items()):
                    if sid_ != sid:
                        continue
                    for handle, stream in readers.items():
                        if handle != packing.cuda_stream:
                            packing.wait_stream(stream)
                    cached = rt._blobs.get(sid)
                    if cached is not None and cached[0] is not blob:
                        rt._retire(sid)              # an image of the stage's own is dropped below: its block stays the readers' until they are through
                    readers.clear()
            _lib.check(L.trajsde_pack_weights_many(self._items, len(self.entries), host.data_ptr(), table.data_ptr(), nbytes, self._fresh,
                                                   _stream()), "trajsde_pack_weights_many")
            self._fresh = 0
            ev = torch.cuda.Event()
            cur = torch.cuda.current_stream()
            ev.record(cur)
        for (rt, sid), stamp, blob in zip(self.entries, stamps, self._blobs):
            rt._blobs[sid] = (blob, stamp, ev, cur.cuda_stream)


def refuse_milstein_training(decoder, local_embed=None, need_embed: bool = False) -> None:
    """a decoder with `method: milstein` trains through the HIP kernels alone (trajsde_decoder_*_backward_milstein): refused where they
    cannot run -- parameters, or the stage input `local_embed` (`need_embed`: it must be given), not on the GPU"""
    if getattr(decoder, "method", "euler") != "milstein":
        return
    first = decoder._rt._first_param()
    missing = need_embed and (local_embed is None or not getattr(local_embed, "is_cuda", False))
    if not first.is_cuda or missing:
        raise NotImplementedError("training a decoder with `method: milstein` runs on the GPU only (the reverse sweep through its gdg term "
                                  "is a HIP kernel): parameters and inputs must be on the GPU")


class StageRuntime:
    """Per-stage glue owned by a stage module (encoder / aggregator / decoder)."""

    STAGE_ID = {"encoder": _lib.STAGE_ENCODER, "aggregator": _lib.STAGE_AGGREGATOR, "decoder": _lib.STAGE_DECODER,
                "encoder_grid": _lib.STAGE_ENCODER_GRID, "decoder_mlp": _lib.STAGE_DECODER_MLP}

    def __init__(self, module, stage: str) -> None:
        object.__setattr__(self, "module", module)
        self.stage = stage
        self.stage_id = self.STAGE_ID[stage]
        self._blobs: Dict[int, tuple] = {}          # stage id -> (blob, parameter stamp, pack-done event, packing stream)
        self._readers: Dict[int, dict] = {}         # stage id -> {stream handle: stream} that read the image from another stream
        self._names: Dict[int, list] = {}

    # ---------------------------------------------------------------- weights
    def _dims(self) -> Tuple[int, int]:
        m = self.module
        if self.stage == "encoder_grid":             # this recipe takes the number of temporal layers
            return int(m.num_temporal_layers), 0
        return int(getattr(m, "num_layers", 0)), int(getattr(m, "num_modes", 0))

    def param_names(self, stage_id: Optional[int] = None):
        stage_id = self.stage_id if stage_id is None else stage_id
        if stage_id not in self._names:
            L = _lib.lib()
            nl, K = self._dims()
            n = L.trajsde_param_count(stage_id, nl, K)
            self._names[stage_id] = [L.trajsde_param_name(stage_id, i, nl, K).decode() for i in range(n)]
        return self._names[stage_id]

    def _first_param(self) -> torch.Tensor:
        """one parameter of the module (its device is the stage's); looked up through the cached slot, not `next(m.parameters())`
        -- that generator walks the module tree, 0.1 ms a call and nine calls a training step"""
        names = self.param_names()
        return self.module.p(names[0]) if names else next(self.module.parameters())

    def _grad_buffers(self, stage_id: int) -> "GradBuffers":
        """zero-initialised gradient buffers of a *_BWD stage as views of ONE flat tensor (one fill instead of one per
        parameter), keyed and ordered like param_names(stage_id)"""
        m = self.module
        lay = self._grad_layouts.get(stage_id) if hasattr(self, "_grad_layouts") else None
        if lay is None:                                                     # names / shapes / offsets do not change: computed once
            names = self.param_names(stage_id)
            lay = GradLayout(names, [tuple(m.p(n).shape) for n in names])
            if not hasattr(self, "_grad_layouts"):
                self._grad_layouts = {}
            self._grad_layouts[stage_id] = lay
        first = self._first_param()
        return GradBuffers(torch.zeros(lay.total, device=first.device, dtype=torch.float32), lay)

    # the parameters do not change between the forward and the backward calls of ONE training step: the path loss pins the stamp
    # for that stretch (pin_stamp / unpin_stamp), so the nine blob() lookups of a step walk the parameter list once per stage
    _pinned_stamp = None

    def pin_stamp(self) -> None:
        self._pinned_stamp = None
        self._pinned_stamp = self._stamp()

    def unpin_stamp(self) -> None:
        self._pinned_stamp = None

    def _stamp(self):
        if self._pinned_stamp is not None:
            return self._pinned_stamp
        return (self.module.version_stamp(), str(self._first_param().device))

    def _param_table(self, stage_id: int):
        """(identity, ctypes array of the parameter addresses, count, blob floats) of a stage's packing -- rebuilt (and the tensors
        re-checked) only when a tensor was replaced or moved: an optimizer step through the flat alias (touch()) re-packs from the
        same addresses"""
        m = self.module
        first = self._first_param()
        walk = m.walk_stamp() if hasattr(m, "walk_stamp") else None
        tab = self._ptr_tables.get(stage_id) if hasattr(self, "_ptr_tables") else None
        if tab is None or walk is None or tab[0] != (walk, str(first.device)):
            L = _lib.lib()
            nl, K = self._dims()
            names = self.param_names(stage_id)
            tensors = []
            for n in names:
                p = m.p(n)
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != first.device:
                    raise _lib.TrajsdeError(f"parameter {self.stage}.{n} must be contiguous fp32 on {first.device}")
                tensors.append(p)
            arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            tab = ((walk, str(first.device)), arr, len(tensors), int(L.trajsde_blob_floats(stage_id, nl, K)))
            if not hasattr(self, "_ptr_tables"):
                self._ptr_tables = {}
            self._ptr_tables[stage_id] = tab
        return tab

    def blob(self, stage_id: Optional[int] = None) -> torch.Tensor:
        """Packed LDS images of this stage's weights (`stage_id`: the forward images by default, or the
        stage's backward images); re-packed whenever a parameter changed."""
        m = self.module
        stage_id = self.stage_id if stage_id is None else stage_id
        first = self._first_param()
        _require_gpu(first, f"{self.stage} parameters")
        stamp = self._stamp()
        cached = self._blobs.get(stage_id)
        if cached is None or stamp != cached[1]:
            L = _lib.lib()
            nl, K = self._dims()
            _, arr, n_tensors, n_floats = self._param_table(stage_id)
            blob = torch.empty(n_floats, device=first.device, dtype=torch.float32)
            self._retire(stage_id)
            with torch.cuda.device(first.device):
                _lib.check(L.trajsde_pack_weights(stage_id, nl, K, arr, n_tensors, blob.data_ptr(), n_floats, _stream()),
                           "trajsde_pack_weights")
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
            self._blobs[stage_id] = (blob, stamp, ev, torch.cuda.current_stream(first.device).cuda_stream)
        blob, stamp_, ev, packed_on = self._blobs[stage_id]
        cur = torch.cuda.current_stream(first.device)
        if cur.cuda_stream != packed_on:
            # a reader on another stream (multi-stream inference, a validation stream beside the training loop): remembered, so that an
            # IN-PLACE re-pack of this image (PackSet.refresh) is ordered behind what the stream still has queued on it
            self._readers.setdefault(stage_id, {})[cur.cuda_stream] = cur
        if ev is not None:
            if ev.query():
                self._blobs[stage_id] = (blob, stamp_, None, packed_on)        # pack finished: nothing left to order against
            elif cur.cuda_stream != packed_on:
                cur.wait_event(ev)          # packed on another stream (multi-stream drivers): order the reads behind the pack
        return blob

    def _retire(self, stage_id: int) -> None:
        """the cached image of `stage_id` is about to be REPLACED by a new tensor: streams that read it from beside its packing stream
        (remembered in `_readers`) may still have kernels queued on it, and they hold a raw pointer -- the caching allocator is told, so
        that the block is not handed out again before they are through.  No host wait; the readers of the new image start afresh."""
        readers = self._readers.pop(stage_id, None)
        cached = self._blobs.get(stage_id)
        if readers and cached is not None:
            for stream in readers.values():
                cached[0].record_stream(stream)

    def packs_complete(self) -> None:
        """the caller has synchronised the device: no pack is in flight, nothing left to order reads against"""
        for sid, (blob, stamp, ev, packed_on) in list(self._blobs.items()):
            self._blobs[sid] = (blob, stamp, None, packed_on)

    # ---------------------------------------------------------------- decoder
    def _decoder_tables(self, T: int, dev):
        """(EulerSchedule, step table, output table) of the SDE decoder's time grid on `dev`, cached per grid"""
        m = self.module
        return _TABLES.get(("dec", T, float(m.max_fut_t), float(m.min_stepsize)),
                           lambda: decoder_schedule(T, float(m.max_fut_t), float(m.min_stepsize)), dev)

    @staticmethod
    def _targets_and_mask(data, out: Dict[str, torch.Tensor], N: int, T: int, what: str):
        """(float32 targets [N,T,2], `reg_mask` as bytes) of the welded losses; `what`: how the error names the targets"""
        y = data["y"]
        if y is None or tuple(y.shape) != (N, T, 2):
            raise _lib.TrajsdeError(f"data['y'] must be [{N},{T},2] ({what})")
        return y.to(torch.float32).contiguous(), out["reg_mask"].contiguous().view(torch.uint8)

    def _backward_outputs(self, stage_id: int, N: int, K: int, dev):
        """what every decoder backward writes: (names, zeroed GradBuffers, their pointer array, d_local [N,64], d_global [K,N,64])"""
        names = self.param_names(stage_id)
        grads = self._grad_buffers(stage_id)
        arr, grads.pointer_keep = grads.pointer_array()                      # (the addresses live as long as the buffers)
        d_local = torch.empty(N, D, device=dev, dtype=torch.float32)
        d_global = torch.empty(K, N, D, device=dev, dtype=torch.float32)
        return names, grads, arr, d_local, d_global

    @staticmethod
    def _cotangents(d_loc: Optional[torch.Tensor], d_pi: Optional[torch.Tensor], K: int, N: int, T: int, dev, allow_two_channels: bool):
        """caller-supplied dL/dloc, dL/dpi -> contiguous float32 [K,N,T,4] and [N,K] on `dev`; None is zeros.  `allow_two_channels`:
        a [K,N,T,2] `d_loc` (the output of `uncertain: False`) is accepted and padded with zero scale channels"""
        if d_loc is None:
            d_loc4 = torch.zeros(K, N, T, 4, device=dev, dtype=torch.float32)
        else:
            if tuple(d_loc.shape) != (K, N, T, 4) and not (allow_two_channels and tuple(d_loc.shape) == (K, N, T, 2)):
                hint = " (or ...,2 without the scale channels)" if allow_two_channels else ""
                raise _lib.TrajsdeError(f"d_loc must be [{K},{N},{T},4]{hint}, got {tuple(d_loc.shape)}")
            d_loc4 = d_loc.detach().to(device=dev, dtype=torch.float32)
            if d_loc4.shape[-1] == 2:                       # `uncertain: False`: no scale channels came out, none carry gradient
                d_loc4 = torch.cat([d_loc4, torch.zeros_like(d_loc4)], dim=-1)
            d_loc4 = d_loc4.contiguous()
        if d_pi is None:
            d_pi_c = torch.zeros(N, K, device=dev, dtype=torch.float32)
        else:
            if tuple(d_pi.shape) != (N, K):
                raise _lib.TrajsdeError(f"d_pi must be [{N},{K}], got {tuple(d_pi.shape)}")
            d_pi_c = d_pi.detach().to(device=dev, dtype=torch.float32).contiguous()
        return d_loc4, d_pi_c

    @staticmethod
    def _checked_ws_bytes(query: str, *args) -> int:
        """a workspace query that can refuse its arguments (a negative size, the reason in trajsde_last_error)"""
        L = _lib.lib()
        ws_bytes = getattr(L, query)(*args)
        if ws_bytes < 0:
            raise _lib.TrajsdeError(f"{query}: {L.trajsde_last_error().decode()}")
        return ws_bytes

    def decoder_forward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor,
                        noise: Optional[NoiseSpec] = None) -> Dict[str, torch.Tensor]:
        m = self.module
        noise = NoiseSpec.resolve(noise)
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        K, T = int(m.num_modes), int(m.future_steps)
        N = local_embed.shape[0]
        sched, step_tab, out_tab = self._decoder_tables(T, dev)
        if noise.z_dec is not None and tuple(noise.z_dec.shape) != (sched.n_euler, K * N, D):
            raise _lib.TrajsdeError(f"z_dec must be [{sched.n_euler},{K * N},{D}] (one increment per Euler step, App. D)")
        L = _lib.lib()
        # `method` (SDEDecoder checks it): euler, or milstein -- the same call on the Milstein image (the decoder blob + GFunc's transposes)
        if m.method == "milstein":
            blob, entry, name = self.blob(_lib.STAGE_DECODER_MILSTEIN), L.trajsde_decoder_forward_milstein, "trajsde_decoder_forward_milstein"
        else:
            blob, entry, name = self.blob(), L.trajsde_decoder_forward, "trajsde_decoder_forward"
        loc = torch.empty(K, N, T, 4, device=dev, dtype=torch.float32)
        pi = torch.empty(N, K, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_decoder_ws_bytes(N, K)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_dec, noise.dec_row_ids)
        with torch.cuda.device(dev):
            _lib.check(entry(N, K, T, blob.data_ptr(), local_embed.contiguous().data_ptr(),
                             global_embed.contiguous().data_ptr(), step_tab.data_ptr(), sched.n_euler,
                             out_tab.data_ptr(), float(m.min_scale), C.byref(cn), ws.data_ptr(), ws_bytes,
                             loc.data_ptr(), pi.data_ptr(), _stream()), name)
        out = {"loc": loc, "pi": pi, "reg_mask": ~data["padding_mask"][:, -T:]}          # DEC:104
        _drop_scale_channels(m, out)
        return out

    def decoder_forward_mc(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, n_samples: int,
                           noise: Optional[NoiseSpec] = None, sample_stride: Optional[int] = None,
                           return_samples: bool = False) -> Dict[str, torch.Tensor]:
        """Monte-Carlo decoding (include/trajsde_hip_mc.h): `n_samples` = R >= 2 sample paths of every (mode, actor) from ONE y0, in one
        launch.  Sample s of path r = k N + n is decoder_forward's solve with the Philox counter row rid(r) + s * D (uint32), D =
        `sample_stride` (default K * N; a sharded caller passes the global row count), so sample 0 is decoder_forward's draw bit for
        bit and sample s is its draw under NoiseSpec(seed, dec_row_ids=ids + s * D).  With `noise.dec_row_ids` the ids stay on the
        device: the caller keeps max(ids) + (R - 1) * D below 2^32 (checked here for local ids only).  `noise.z_dec`, if given, is
        [n_euler, R * K * N, 64], row s * K * N + r.  Returns `loc` (sample 0, as decoder_forward returns it: the entry point's `loc0`
        output, no second solve), `pi`, `reg_mask`, `loc_mean` [K,N,T,4] (sample mean of x, y, scale_x, scale_y), `loc_cov` [K,N,T,3]
        (unbiased var_x, var_y, cov_xy) and, with `return_samples`, `samples` [R,K,N,T,4].  `uncertain: False` drops the scale channels
        of `loc`, `loc_mean` and `samples`.  No host synchronisation; `noise.seed_dev` is honoured."""
        m = self.module
        K, T = int(m.num_modes), int(m.future_steps)
        N = local_embed.shape[0]
        R, stride = mc_check_arguments(n_samples, K * N, sample_stride)
        noise = NoiseSpec.resolve(noise)
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        sched, step_tab, out_tab = self._decoder_tables(T, dev)
        if noise.z_dec is not None and tuple(noise.z_dec.shape) != (sched.n_euler, R * K * N, D):
            raise _lib.TrajsdeError(f"z_dec must be [{sched.n_euler},{R * K * N},{D}] (n_samples * K * N rows per Euler step, sample-major)")
        L = _lib.lib()
        milstein = m.method == "milstein"
        blob = self.blob(_lib.STAGE_DECODER_MILSTEIN) if milstein else self.blob()
        loc = torch.empty(K, N, T, 4, device=dev, dtype=torch.float32)
        loc_mean = torch.empty(K, N, T, 4, device=dev, dtype=torch.float32)
        loc_cov = torch.empty(K, N, T, 3, device=dev, dtype=torch.float32)
        samples = torch.empty(R, K, N, T, 4, device=dev, dtype=torch.float32) if return_samples else None
        pi = torch.empty(N, K, device=dev, dtype=torch.float32)
        ws_bytes = self._checked_ws_bytes("trajsde_decoder_mc_ws_bytes", N, K, T, R)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_dec, noise.dec_row_ids)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_decoder_forward_mc(N, K, T, 1 if milstein else 0, blob.data_ptr(), local_embed.contiguous().data_ptr(),
                                                    global_embed.contiguous().data_ptr(), step_tab.data_ptr(), sched.n_euler,
                                                    out_tab.data_ptr(), float(m.min_scale), C.byref(cn), R, stride, ws.data_ptr(), ws_bytes,
                                                    loc_mean.data_ptr(), loc_cov.data_ptr(), _ptr(samples), loc.data_ptr(), pi.data_ptr(),
                                                    _stream()), "trajsde_decoder_forward_mc")
        out = {"loc": loc, "pi": pi, "reg_mask": ~data["padding_mask"][:, -T:], "loc_mean": loc_mean, "loc_cov": loc_cov}
        if samples is not None:
            out["samples"] = samples
        _drop_scale_channels(m, out)
        if not getattr(m, "uncertain", True):
            out["loc_mean"] = loc_mean[..., :2].contiguous()
            if samples is not None:
                out["samples"] = samples[..., :2].contiguous()
        return out

    def decoder_nll_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                             noise: NoiseSpec, eps: float = 1e-6) -> Dict[str, object]:
        """Laplace negative log-likelihood of the winning mode (losses/laplace_nll_loss.py:18-47) on `out` = decoder_forward(...)
        and its gradients -- like decoder_l2_backward, with the scale head differentiated as well (grads keyed by
        param_names(STAGE_DECODER_NLL_BWD))."""
        return self._decoder_backward(data, local_embed, global_embed, out, noise, nll_eps=float(eps))

    def decoder_l2_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                            noise: NoiseSpec) -> Dict[str, object]:
        """Winner-takes-all L2 loss (losses/L2.py:10-27) on `out` = decoder_forward(...) and its gradients w.r.t.
        this stage's parameters and inputs.  `noise` must be the NoiseSpec the forward ran with (same seed / z), so
        that the replayed winning paths are the forward's.  Returns {"loss", "best_mode", "grads": {param name:
        tensor}, "d_local_embed", "d_global_embed"}; `pi.*` and `scale.*` get no gradient from this loss."""
        return self._decoder_backward(data, local_embed, global_embed, out, noise, nll_eps=None)

    def _decoder_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                          noise: NoiseSpec, nll_eps: Optional[float]) -> Dict[str, object]:
        """shared body of decoder_l2_backward / decoder_nll_backward (`nll_eps` None: L2); `method: milstein` takes the Milstein
        entry points on the Milstein images (the forward's, and the backward's with GFunc's tangent images appended)"""
        refuse_milstein_training(self.module, local_embed, need_embed=True)
        m = self.module
        if noise is None:
            raise _lib.TrajsdeError("decoder_l2_backward needs the NoiseSpec of the forward pass (seed or z_dec)")
        if nll_eps is not None and not getattr(m, "uncertain", True):
            raise _lib.TrajsdeError("LaplaceNLLLoss needs the decoder's scale head: `uncertain: False` has none (DEC:56, "
                                    "losses/laplace_nll_loss.py:28 chunks loc | scale out of four channels)")
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        K, T = int(m.num_modes), int(m.future_steps)
        N = local_embed.shape[0]
        sched, step_tab, out_tab = self._decoder_tables(T, dev)
        y, mask = self._targets_and_mask(data, out, N, T, "rotated targets, MODEL:83-84")
        L = _lib.lib()
        stage = _lib.STAGE_DECODER_BWD if nll_eps is None else _lib.STAGE_DECODER_NLL_BWD
        names, grads, arr, d_local, d_global = self._backward_outputs(stage, N, K, dev)
        milstein = m.method == "milstein"
        if milstein:                       # (the same parameter tables: the gradient buffers and their order are the Euler ones)
            fwd_stage = _lib.STAGE_DECODER_MILSTEIN
            blob_stage = _lib.STAGE_DECODER_MILSTEIN_BWD if nll_eps is None else _lib.STAGE_DECODER_MILSTEIN_NLL_BWD
        else:
            fwd_stage, blob_stage = self.stage_id, stage
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        best = torch.empty(N, device=dev, dtype=torch.int32)
        cn = noise.c_noise(noise.z_dec, noise.dec_row_ids)
        head = (N, K, T, self.blob(fwd_stage).data_ptr(), self.blob(blob_stage).data_ptr(),
                local_embed.contiguous().data_ptr(), global_embed.contiguous().data_ptr(), step_tab.data_ptr(), sched.n_euler,
                out_tab.data_ptr(), C.byref(cn), _loc4(out).data_ptr(), y.data_ptr(), mask.data_ptr())
        sfx = "_milstein" if milstein else ""
        if milstein:                                     # (one workspace query covers both losses)
            ws_query = L.trajsde_decoder_milstein_backward_ws_bytes
        else:
            ws_query = L.trajsde_decoder_backward_ws_bytes if nll_eps is None else L.trajsde_decoder_nll_backward_ws_bytes
        ws_bytes = ws_query(N, K, T, sched.n_euler)
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            if nll_eps is None:
                name = "trajsde_decoder_l2_backward" + sfx
                _lib.check(getattr(L, name)(*head, ws.data_ptr(), ws_bytes, loss.data_ptr(), best.data_ptr(), arr, len(names),
                                            d_local.data_ptr(), d_global.data_ptr(), _stream()), name)
            else:
                name = "trajsde_decoder_nll_backward" + sfx
                _lib.check(getattr(L, name)(*head, float(nll_eps), float(m.min_scale), ws.data_ptr(), ws_bytes, loss.data_ptr(),
                                            best.data_ptr(), arr, len(names), d_local.data_ptr(), d_global.data_ptr(), _stream()), name)
        return {"loss": loss[0], "best_mode": best, "grads": grads, "d_local_embed": d_local, "d_global_embed": d_global}

    def decoder_cotangent_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                                   noise: NoiseSpec, d_loc: Optional[torch.Tensor], d_pi: Optional[torch.Tensor],
                                   support: str = "all") -> Dict[str, object]:
        """Vector-Jacobian product of the decoder stage (DEC:77-105, Euler-Maruyama) at the forward's noise, from caller-supplied
        cotangents: `d_loc` = dL/dloc [K,N,T,4] (or [K,N,T,2] without the scale head) and `d_pi` = dL/dpi [N,K] of ANY loss over all K
        modes; None is zeros.  `out` = decoder_forward(...), `noise` the NoiseSpec it ran with.  Every one of the K * N paths is
        replayed and swept in reverse, so the workspace is about K times decoder_l2_backward's.  Returns {"grads": {param name:
        tensor} keyed by param_names(STAGE_DECODER_COT_BWD) -- `scale.*` and `pi.*` included --, "d_local_embed", "d_global_embed"}.
        `support="winner"` (trajsde_decoder_cotangent_backward_sel) is for a `d_loc` that is non-zero in at most one mode per actor, as a
        winner-takes-all regression loss leaves it: that mode is found on the device and only its path is replayed and swept, so the
        SDE tape is decoder_nll_backward's whatever K is; `pi` is differentiated over all K modes as before.  The result then also holds
        "support_status", a device tensor of two int32 (actors with more than one supported mode -- the premise is violated unless this is
        0, and the gradients are then those of each actor's lowest supported mode alone --, actors with any support) and
        "support_mode" [N] int32, the selected modes; no host synchronisation is added, reading them is the caller's."""
        if support not in ("all", "winner"):
            raise ValueError(f"support {support!r}: 'all' (every one of the K * N paths) or 'winner' (each actor's one supported mode)")
        m = self.module
        if getattr(m, "method", "euler") == "milstein":
            raise NotImplementedError("decoder_cotangent_backward differentiates the Euler-Maruyama solve only: `method: milstein` trains "
                                      "under L2 or LaplaceNLLLoss (+ DiffBCE), whose backward is fused with the Milstein sweep")
        if noise is None:
            raise _lib.TrajsdeError("decoder_cotangent_backward needs the NoiseSpec of the forward pass (seed or z_dec)")
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        K, T = int(m.num_modes), int(m.future_steps)
        N = local_embed.shape[0]
        sched, step_tab, out_tab = self._decoder_tables(T, dev)
        loc4 = _loc4(out)
        d_loc4, d_pi_c = self._cotangents(d_loc, d_pi, K, N, T, dev, allow_two_channels=True)
        L = _lib.lib()
        stage = _lib.STAGE_DECODER_COT_BWD
        names, grads, arr, d_local, d_global = self._backward_outputs(stage, N, K, dev)
        cn = noise.c_noise(noise.z_dec, noise.dec_row_ids)
        name = "trajsde_decoder_cotangent_backward" + ("_sel" if support == "winner" else "")
        ws_bytes = self._checked_ws_bytes(name + "_ws_bytes", N, K, T, sched.n_euler)
        res = {"grads": grads, "d_local_embed": d_local, "d_global_embed": d_global}
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            tail = (_stream(),)
            if support == "winner":
                res["support_status"] = torch.empty(2, device=dev, dtype=torch.int32)
                res["support_mode"] = ws[:4 * N].view(torch.int32)          # (the selection: the workspace's first N words)
                tail = (res["support_status"].data_ptr(), _stream())
            _lib.check(getattr(L, name)(
                N, K, T, self.blob().data_ptr(), self.blob(stage).data_ptr(), local_embed.contiguous().data_ptr(),
                global_embed.contiguous().data_ptr(), step_tab.data_ptr(), sched.n_euler, out_tab.data_ptr(), C.byref(cn),
                loc4.data_ptr(), float(m.min_scale), d_loc4.data_ptr(), d_pi_c.data_ptr(), ws.data_ptr(), ws_bytes, arr, len(names),
                d_local.data_ptr(), d_global.data_ptr(), *tail), name)
        return res

    # ---------------------------------------------------------------- encoder
    def encoder_forward(self, data, noise: Optional[NoiseSpec] = None, preserve_side_effects: bool = False):
        """LocalEncoderSDESepPara2.forward (ENC:66-202) -> (local_embed, diff_in, diff_out, label_in, label_out).
        `preserve_side_effects`: also leave `edge_index_{t}` / `edge_attr_{t}` on the batch like ENC:107-110 does."""
        m = self.module
        noise = NoiseSpec.resolve(noise)
        cap = bool(getattr(m, "capture_intermediates", False))
        L = _lib.lib()
        prev = L.trajsde_export_senders(1) if cap else 0                  # edge lists with their senders, for the tests
        try:
            gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise, want_senders=cap,
                                  exact=True if cap else not sync_free())
        finally:
            if cap:
                L.trajsde_export_senders(prev)
        dev = gc.device
        blob = self.blob()
        H, N, A, Nt = gc.batch.H, gc.batch.N, gc.batch.A, gc.graph.Nt
        tab = self._enc_table()
        if noise.z_enc is not None and tuple(noise.z_enc.shape) != (H, Nt, D):
            raise _lib.TrajsdeError(f"z_enc must be [{H},{Nt},{D}]")
        local = torch.empty(N, D, device=dev, dtype=torch.float32)
        diff_pick = torch.empty(2 * A, D, device=dev, dtype=torch.float32)
        aa_out = torch.empty(H, Nt, D, device=dev, dtype=torch.float32) if cap else None
        latent = torch.empty(H, N, D, device=dev, dtype=torch.float32) if cap else None
        ws_bytes = L.trajsde_encoder_ws_bytes(C.byref(gc.batch), C.byref(gc.graph))
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_enc, noise.enc_row_ids)
        dr = noise.c_dropout(m)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_encoder_forward(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), blob.data_ptr(),
                                                 tab.ctypes.data_as(C.c_void_p), C.byref(cn), ws.data_ptr(), ws_bytes,
                                                 local.data_ptr(), diff_pick.data_ptr(), _ptr(aa_out), _ptr(latent),
                                                 C.byref(dr) if dr is not None else None, _stream()),
                       "trajsde_encoder_forward")
        if cap:
            if state_storage() == "bf16":                                  # aa_out was written with 2-byte elements
                aa_out = aa_out.view(-1).view(torch.bfloat16)[:H * Nt * D].view(H, Nt, D).float()
            m.last_intermediates = {"aa_out": aa_out, "latent_ys": latent, **gc.true_counts(), **gc.edge_lists()}
        if preserve_side_effects:
            edge_snapshots(data, H)                                                         # ENC:107-110
        diff_in, diff_out = torch.chunk(diff_pick, 2, 0)                                    # ENC:194
        return (local, diff_in, diff_out, torch.full_like(diff_in, m.real_label), torch.full_like(diff_out, m.fake_label))

    def encoder_forward_train(self, data, noise: NoiseSpec):
        """The encoder's forward for a training step: same outputs as encoder_forward (same weights, noise, dropout), computed
        by the kernels that keep the tape the backward needs.  Returns (outputs tuple, tape) -- hand `tape` to encoder_backward
        and the backward does not recompute the forward."""
        m = self.module
        gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise)
        dev = gc.device
        L = _lib.lib()
        N, A = gc.batch.N, gc.batch.A
        tab = self._enc_table()
        local = torch.empty(N, D, device=dev, dtype=torch.float32)
        diff_pick = torch.empty(2 * A, D, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_encoder_tape_bytes(C.byref(gc.batch), C.byref(gc.graph))
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_enc, noise.enc_row_ids)
        dr = noise.c_dropout(m)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_encoder_forward_train(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), self.blob().data_ptr(),
                                                       tab.ctypes.data_as(C.c_void_p), C.byref(cn), ws.data_ptr(), ws_bytes, local.data_ptr(),
                                                       diff_pick.data_ptr(), C.byref(dr) if dr is not None else None, _stream()),
                       "trajsde_encoder_forward_train")
        diff_in, diff_out = torch.chunk(diff_pick, 2, 0)
        outs = (local, diff_in, diff_out, torch.full_like(diff_in, m.real_label), torch.full_like(diff_out, m.fake_label))
        return outs, (ws, ws_bytes)

    def encoder_backward(self, data, d_local: torch.Tensor, noise: NoiseSpec, diff_weight: float = 1.0,
                         want_boundaries: bool = False, tape=None, keep_scratch: bool = False) -> Dict[str, object]:
        """Backward of LocalEncoderSDESepPara2.forward plus the DiffBCE term: `d_local` = dL/d local_embed [N,64],
        `noise` the forward's NoiseSpec.  Returns {"grads": {param name: tensor}, "diff_loss": diff_weight * DiffBCE}
        (+ "d_latent" [N,64], "d_aa_out" [H,Nt,64] with want_boundaries).  `tape`: what encoder_forward_train returned for
        this very step; without it the forward is recomputed inside.  `keep_scratch` (reproducibility checks): the backward's
        scratch buffer starts zeroed and is returned as "_scratch"."""
        return self._encoder_backward(data, d_local, noise, want_boundaries, tape, keep_scratch, diff_weight=diff_weight)

    def encoder_cotangent_backward(self, data, d_local: Optional[torch.Tensor], d_diff_in: Optional[torch.Tensor],
                                   d_diff_out: Optional[torch.Tensor], noise: NoiseSpec, tape=None,
                                   want_boundaries: bool = False) -> Dict[str, object]:
        """Vector-Jacobian product of LocalEncoderSDESepPara2.forward at the forward's noise, from caller-supplied cotangents of its
        three differentiable outputs (trajsde_encoder_cotangent_backward): `d_local` = dL/d local_embed [N,64], `d_diff_in` /
        `d_diff_out` = dL/d diff_in, dL/d diff_out [A,64]; None is zeros.  No loss is formed inside.  Returns {"grads": {param name:
        tensor}} keyed by param_names(STAGE_ENCODER_BWD) (+ "d_latent", "d_aa_out" with want_boundaries); `tape` as in
        encoder_backward."""
        return self._encoder_backward(data, d_local, noise, want_boundaries, tape, False, cotangents=(d_diff_in, d_diff_out))

    def _encoder_backward(self, data, d_local: Optional[torch.Tensor], noise: NoiseSpec, want_boundaries: bool, tape, keep_scratch: bool,
                          diff_weight: Optional[float] = None, cotangents=None) -> Dict[str, object]:
        """shared body of encoder_backward (`diff_weight`: DiffBCE welded in) and encoder_cotangent_backward (`cotangents`: dL/d diff_in,
        dL/d diff_out): gradient buffers, tape, the scratch allocated late"""
        m = self.module
        what = "encoder_backward" if cotangents is None else "encoder_cotangent_backward"
        if noise is None:
            raise _lib.TrajsdeError(f"{what} needs the NoiseSpec of the forward pass")
        gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise)
        dev = gc.device
        L = _lib.lib()
        H, N, A, Nt = gc.batch.H, gc.batch.N, gc.batch.A, gc.graph.Nt
        if d_local is None and cotangents is not None:
            d_local = torch.zeros(N, D, device=dev, dtype=torch.float32)
        if tuple(d_local.shape) != (N, D):
            raise _lib.TrajsdeError(f"d_local must be [{N},{D}]")
        if cotangents is not None:
            _require_gpu(d_local, "d_local")
            cots = []
            for name, t in zip(("d_diff_in", "d_diff_out"), cotangents):
                if t is not None:
                    if tuple(t.shape) != (A, D):
                        raise _lib.TrajsdeError(f"{name} must be [{A},{D}], got {tuple(t.shape)}")
                    _require_gpu(t, name)
                    t = t.detach().to(torch.float32).contiguous()
                cots.append(t)
        tab = self._enc_table()
        tab_dev = _TABLES_DEV.get((id(tab), str(dev)))                     # (not setdefault: its default would be built -- a blocking
        if tab_dev is None:                                                #  pageable host-to-device copy -- on every call)
            tab_dev = _TABLES_DEV[(id(tab), str(dev))] = torch.from_numpy(tab).to(dev)
        names = self.param_names(_lib.STAGE_ENCODER_BWD)
        grads = self._grad_buffers(_lib.STAGE_ENCODER_BWD)
        arr, _keep = grads.pointer_array()
        loss = torch.empty(1, device=dev, dtype=torch.float32) if cotangents is None else None
        d_lat = torch.empty(N, D, device=dev, dtype=torch.float32) if want_boundaries else None
        d_aa = torch.empty(H, Nt, D, device=dev, dtype=torch.float32) if want_boundaries else None
        if tape is not None:
            ws, ws_bytes = tape
        else:
            ws_bytes = L.trajsde_encoder_tape_bytes(C.byref(gc.batch), C.byref(gc.graph))
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        # the backward's own scratch is a separate buffer, allocated only now: between the training forward and this call the
        # step holds the tape alone, and the decoder's / aggregator's workspaces have been released by the time this one is taken
        sc_bytes = L.trajsde_encoder_backward_scratch_bytes(C.byref(gc.batch), C.byref(gc.graph))
        scratch = (torch.zeros if keep_scratch else torch.empty)(sc_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_enc, noise.enc_row_ids)
        dr = noise.c_dropout(m)                                            # the forward's masks, regenerated from the same key
        d_local_c = d_local.to(torch.float32).contiguous()
        head = (C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), self.blob().data_ptr(),
                self.blob(_lib.STAGE_ENCODER_BWD).data_ptr(), tab.ctypes.data_as(C.c_void_p), tab_dev.data_ptr(), C.byref(cn),
                d_local_c.data_ptr())
        tail = (arr, len(names), _ptr(d_lat), _ptr(d_aa), C.byref(dr) if dr is not None else None, 1 if tape is not None else 0,
                scratch.data_ptr(), sc_bytes, _stream())
        with torch.cuda.device(dev):
            if cotangents is None:
                _lib.check(L.trajsde_encoder_backward(*head, float(diff_weight), ws.data_ptr(), ws_bytes, loss.data_ptr(), *tail),
                           "trajsde_encoder_backward")
            else:
                _lib.check(L.trajsde_encoder_cotangent_backward(*head, _ptr(cots[0]), _ptr(cots[1]), ws.data_ptr(), ws_bytes, *tail),
                           "trajsde_encoder_cotangent_backward")
        out = {"grads": grads}
        if cotangents is None:
            out["diff_loss"] = loss[0]
        if want_boundaries:
            out.update(d_latent=d_lat, d_aa_out=d_aa)
        if keep_scratch:
            out["_scratch"] = scratch
        return out

    def _enc_table(self) -> np.ndarray:
        m = self.module
        key = (int(m.historical_steps), float(m.max_past_t), float(m.minimum_step), bool(m.run_backwards))
        if key not in _ENC_TABLES:               # host replay of the solver's float32 time bookkeeping: once per config
            sched = encoder_schedule(*key)
            if sched.n_euler != key[0] or not np.all(sched.out_w1 == 1.0):
                raise _lib.TrajsdeError("encoder schedule is not one Euler step per interval (SURVEY App. D)")
            _ENC_TABLES[key] = np.ascontiguousarray(sched.step_table())
        return _ENC_TABLES[key]

    def encoder_forward_ood(self, data, noise: Optional[NoiseSpec] = None, n_samples: int = 10):
        """LocalEncoderSDESepPara2.forward_ood (ENC:204-370) -> (local_embed, actors_std)."""
        m = self.module
        noise = NoiseSpec.resolve(noise)
        gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), noise, fake_agents=False, exact=not sync_free())
        dev = gc.device
        L = _lib.lib()
        blob = self.blob()
        H, N = gc.batch.H, gc.batch.N
        tab = self._enc_table()
        if noise.z_enc is not None and tuple(noise.z_enc.shape) != (n_samples * H, N, D):
            raise _lib.TrajsdeError(f"z_enc must be [{n_samples * H},{N},{D}] for forward_ood")
        local = torch.empty(N, D, device=dev, dtype=torch.float32)
        stds = torch.empty(N, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_encoder_ood_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), n_samples)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        cn = noise.c_noise(noise.z_enc, noise.enc_row_ids)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_encoder_forward_ood(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), blob.data_ptr(),
                                                     tab.ctypes.data_as(C.c_void_p), C.byref(cn), n_samples, ws.data_ptr(), ws_bytes,
                                                     local.data_ptr(), stds.data_ptr(), _stream()), "trajsde_encoder_forward_ood")
        return local, stds

    # ---------------------------------------------------------------- aggregator
    def aggregator_forward(self, data, local_embed: torch.Tensor, noise: Optional[NoiseSpec] = None,
                           prepared: Optional["RelPrefetch"] = None) -> torch.Tensor:
        """GlobalInteractor.forward (AGG:38-58) -> [K, N, 64].  `noise`: only its dropout key is used, in train mode.
        `prepared`: what `prefetch_rel_embed` returned for this forward -- the relative-pose rows are then already in the
        workspace (or on their way on the side stream: this stream waits for them) and the call skips that kernel."""
        m = self.module
        dr = NoiseSpec.resolve(noise).c_dropout(m) if (m.training and float(getattr(m, "dropout", 0.0) or 0.0) > 0) else None
        _require_gpu(local_embed, "local_embed")
        gc = GraphContext.get(data, None, int(m.historical_steps), None, exact=None)
        dev = gc.device
        L = _lib.lib()
        blob = self.blob()
        K, N = int(m.num_modes), gc.batch.N
        out = torch.empty(K, N, D, device=dev, dtype=torch.float32)
        if prepared is not None and prepared.gc is not gc:
            prepared.join()                                               # (the graph was rebuilt in between: the rows are of another list)
            prepared = None
        if prepared is not None:
            ws, ws_bytes = prepared.ws, prepared.ws_bytes
            prepared.join()
            entry = L.trajsde_aggregator_forward_prepared
        else:
            ws_bytes = L.trajsde_aggregator_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), K)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            entry = L.trajsde_aggregator_forward_heads
        with torch.cuda.device(dev):
            _lib.check(entry(C.byref(gc.batch), C.byref(gc.graph), blob.data_ptr(), int(m.num_layers), K,
                             int(m.num_heads), local_embed.contiguous().data_ptr(), ws.data_ptr(),
                             ws_bytes, out.data_ptr(), C.byref(dr) if dr is not None else None, _stream()),
                       "trajsde_aggregator_forward")
        return out

    def arm_rel_prefetch(self, data, encoder_module) -> Optional["torch.cuda.Stream"]:
        """Called on the AGGREGATOR's runtime before the encoder of an inference forward: names the side stream on which the
        relative-pose embedding (AGG:42-51; it reads the graph stage's output only) will run, and has the encoder call fork it
        at the point where its recurrence starts (trajsde_encoder_fork_stream).  That kernel fills the chip for ~0.2 ms and depends
        on nothing the encoder computes, while the recurrence keeps a third of the CUs idle at one wave per SIMD for about as
        long.  None when switched off (the default; TRAJSDE_OVERLAP_REL=1 turns it on) or where the split entry points do not apply."""
        if not _OVERLAP_REL:
            return None
        m, enc = self.module, encoder_module
        if bool(getattr(enc, "capture_intermediates", False)) or m.training or enc.training:
            return None
        x = data["x"]
        _require_gpu(x, "data['x']")
        side = _side_stream(x.device, torch.cuda.current_stream(x.device))
        _lib.check(_lib.lib().trajsde_encoder_fork_stream(side.cuda_stream), "trajsde_encoder_fork_stream")
        return side

    def launch_rel_prefetch(self, data, side) -> Optional["RelPrefetch"]:
        """after the encoder call returned: the side stream now waits for the fork event; enqueue the embedding on it"""
        if side is None or GraphContext.KEY not in data:
            return None
        m = self.module
        gc = GraphContext.get(data, None, int(m.historical_steps), None, exact=None)
        dev = gc.device
        L = _lib.lib()
        blob = self.blob()                                                # (packed on the current stream before the side kernel reads it:
        ws_bytes = L.trajsde_aggregator_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), int(m.num_modes))     # see pack event below)
        packed = self._blobs[self.stage_id][2]                            # a pack still in flight on another stream: order behind it
        cur = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(side):
            # the workspace comes from the SIDE stream's share of the caching allocator: a block of the current stream's could be
            # the encoder workspace that was released a moment ago on the host while the encoder's kernels -- beside which the
            # side kernel is about to run -- still use it
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            if packed is not None:
                side.wait_event(packed)
            _lib.check(L.trajsde_aggregator_prepare(C.byref(gc.batch), C.byref(gc.graph), blob.data_ptr(), ws.data_ptr(), ws_bytes,
                                                    side.cuda_stream), "trajsde_aggregator_prepare")
            done = torch.cuda.Event()
            done.record(side)
        ws.record_stream(cur)                                             # ... and is used on the current stream from the join on
        return RelPrefetch(gc, ws, ws_bytes, done, dev)

    # ---------------------------------------------------------------- vanilla HiVT variant
    def encoder_grid_forward(self, data, noise: Optional[NoiseSpec] = None, exact: bool = False) -> torch.Tensor:
        """LocalEncoder.forward (enc_hivt_nusargo_grid.py:52-93) -> local_embed [N,64].  In train mode the module's `dropout` is
        applied at the reference's sites with masks keyed by `noise` (csrc/dropout.hpp); the variant draws no other noise.
        `exact`: the caller is a training forward (training_step, a stage autograd node) whose backward needs the list lengths on the
        host anyway -- the graph is built exact; otherwise it is built sync-free (lengths on the device) like encoder_forward's."""
        m = self.module
        dr = noise.c_dropout(m) if noise is not None else None
        if dr is None and m.training and float(getattr(m, "dropout", 0.0) or 0.0) > 0:
            raise _lib.TrajsdeError("encoder_grid_forward in train mode needs a NoiseSpec (dropout key)")
        gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), NoiseSpec(seed=0), fake_agents=False,   # no fake agents: the graph only
                              exact=True if exact else not sync_free())
        dev = gc.device
        L = _lib.lib()
        blob = self.blob()
        N = gc.batch.N
        local = torch.empty(N, D, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_encoder_grid_ws_bytes(C.byref(gc.batch), C.byref(gc.graph))
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_encoder_grid_forward_train(C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), blob.data_ptr(),
                                                            int(m.num_heads), int(m.num_temporal_layers), ws.data_ptr(), ws_bytes,
                                                            local.data_ptr(), C.byref(dr) if dr is not None else None, _stream()),
                       "trajsde_encoder_grid_forward_train")
        return local

    def encoder_grid_backward(self, data, d_local: torch.Tensor, noise: Optional[NoiseSpec] = None) -> Dict[str, object]:
        """backward of the vanilla LocalEncoder: dL/d local_embed [N,64] -> {"grads": {param name: tensor}}; `noise`: the forward's
        (train mode: its dropout key -- the masks are regenerated)"""
        m = self.module
        dr = noise.c_dropout(m) if noise is not None else None
        if dr is None and m.training and float(getattr(m, "dropout", 0.0) or 0.0) > 0:
            raise _lib.TrajsdeError("encoder_grid_backward in train mode needs the NoiseSpec of the forward pass (dropout key)")
        gc = GraphContext.get(data, float(m.local_radius), int(m.historical_steps), NoiseSpec(seed=0), fake_agents=False)
        dev = gc.device
        L = _lib.lib()
        N, nl = gc.batch.N, int(m.num_temporal_layers)
        if tuple(d_local.shape) != (N, D):
            raise _lib.TrajsdeError(f"d_local must be [{N},{D}]")
        names = self.param_names(_lib.STAGE_ENCODER_GRID_BWD)
        grads = self._grad_buffers(_lib.STAGE_ENCODER_GRID_BWD)
        arr, _keep = grads.pointer_array()
        ws_bytes = L.trajsde_encoder_grid_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), nl)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_encoder_grid_backward_train(
                C.byref(gc.batch), C.byref(gc.graph), gc.rot.data_ptr(), self.blob().data_ptr(),
                self.blob(_lib.STAGE_ENCODER_GRID_BWD).data_ptr(), int(m.num_heads), nl,
                d_local.to(torch.float32).contiguous().data_ptr(), ws.data_ptr(), ws_bytes, arr, len(names),
                C.byref(dr) if dr is not None else None, _stream()), "trajsde_encoder_grid_backward_train")
        return {"grads": grads}

    def mlp_decoder_forward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor) -> Dict[str, torch.Tensor]:
        """MLPDecoder.forward (dec_hivt_nusargo_grid.py:47-63)"""
        m = self.module
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        K, T, N = int(m.num_modes), int(m.future_steps), local_embed.shape[0]
        L = _lib.lib()
        blob = self.blob()
        loc = torch.empty(K, N, T, 4, device=dev, dtype=torch.float32)
        pi = torch.empty(N, K, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_mlp_decoder_ws_bytes(N, K)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_mlp_decoder_forward(N, K, T, blob.data_ptr(), local_embed.contiguous().data_ptr(),
                                                     global_embed.contiguous().data_ptr(), float(m.min_scale), ws.data_ptr(),
                                                     ws_bytes, loc.data_ptr(), pi.data_ptr(), _stream()),
                       "trajsde_mlp_decoder_forward")
        out = {"loc": loc, "pi": pi, "reg_mask": ~data["padding_mask"][:, -T:]}
        if getattr(m, "uncertain", True):                    # (the reference returns the embeddings on this branch only, :56-57)
            out["local_embed"], out["global_embed"] = local_embed, global_embed
        _drop_scale_channels(m, out)
        return out


    def aggregator_forward_train(self, data, local_embed: torch.Tensor, noise: Optional[NoiseSpec] = None):
        """GlobalInteractor.forward for a training step -> (global_embed [K,N,64], tape for aggregator_backward)"""
        m = self.module
        _require_gpu(local_embed, "local_embed")
        gc = GraphContext.get(data, None, int(m.historical_steps), None)
        dev = gc.device
        L = _lib.lib()
        K, N, nl = int(m.num_modes), gc.batch.N, int(m.num_layers)
        out = torch.empty(K, N, D, device=dev, dtype=torch.float32)
        ws_bytes = L.trajsde_aggregator_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), nl, K)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        dr = noise.c_dropout(m) if noise is not None else None
        if dr is None and m.training and float(getattr(m, "dropout", 0.0) or 0.0) > 0:
            raise _lib.TrajsdeError("aggregator_forward_train in train mode needs a NoiseSpec (dropout key)")
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_aggregator_forward_train(C.byref(gc.batch), C.byref(gc.graph), self.blob().data_ptr(), nl, K, int(m.num_heads),
                                                          local_embed.contiguous().data_ptr(), ws.data_ptr(), ws_bytes, out.data_ptr(),
                                                          C.byref(dr) if dr is not None else None, _stream()), "trajsde_aggregator_forward_train")
        return out, (ws, ws_bytes)

    def aggregator_backward(self, data, local_embed: torch.Tensor, d_global: torch.Tensor,
                            noise: Optional[NoiseSpec] = None, tape=None) -> Dict[str, object]:
        """Backward of GlobalInteractor.forward: dL/d global_embed [K,N,64] -> {"grads": {param name: tensor},
        "d_local_embed": [N,64]} (the aggregator's own contribution; the decoder's d local_embed is added by the
        caller).  The forward is recomputed inside the call."""
        m = self.module
        _require_gpu(local_embed, "local_embed")
        gc = GraphContext.get(data, None, int(m.historical_steps), None)
        dev = gc.device
        L = _lib.lib()
        K, N, nl = int(m.num_modes), gc.batch.N, int(m.num_layers)
        if tuple(d_global.shape) != (K, N, D):
            raise _lib.TrajsdeError(f"d_global must be [{K},{N},{D}]")
        names = self.param_names(_lib.STAGE_AGGREGATOR_BWD)
        grads = self._grad_buffers(_lib.STAGE_AGGREGATOR_BWD)
        arr, _keep = grads.pointer_array()
        d_local = torch.empty(N, D, device=dev, dtype=torch.float32)
        if tape is not None:
            ws, ws_bytes = tape
        else:
            ws_bytes = L.trajsde_aggregator_backward_ws_bytes(C.byref(gc.batch), C.byref(gc.graph), nl, K)
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        dr = noise.c_dropout(m) if noise is not None else None            # the forward's masks
        if dr is None and m.training and float(getattr(m, "dropout", 0.0) or 0.0) > 0:
            raise _lib.TrajsdeError("aggregator_backward in train mode needs the NoiseSpec of the forward pass (dropout key)")
        with torch.cuda.device(dev):
            _lib.check(L.trajsde_aggregator_backward_heads(
                C.byref(gc.batch), C.byref(gc.graph), self.blob().data_ptr(), self.blob(_lib.STAGE_AGGREGATOR_BWD).data_ptr(), nl, K,
                int(m.num_heads), local_embed.contiguous().data_ptr(), d_global.to(torch.float32).contiguous().data_ptr(), ws.data_ptr(), ws_bytes,
                arr, len(names), d_local.data_ptr(), C.byref(dr) if dr is not None else None, 1 if tape is not None else 0, _stream()),
                "trajsde_aggregator_backward")
        return {"grads": grads, "d_local_embed": d_local}


    def mlp_decoder_l2_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor,
                                out: Dict[str, torch.Tensor]) -> Dict[str, object]:
        """L2 (winner takes all) on `out` = mlp_decoder_forward(...) and its gradients, like decoder_l2_backward"""
        return self._mlp_decoder_backward(data, local_embed, global_embed, out, nll_eps=None)

    def mlp_decoder_nll_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor,
                                 out: Dict[str, torch.Tensor], eps: float = 1e-6) -> Dict[str, object]:
        """Laplace negative log-likelihood of the winning mode (losses/laplace_nll_loss.py:18-47) on `out` = mlp_decoder_forward(...)
        and its gradients -- like mlp_decoder_l2_backward, with the scale head differentiated as well (grads keyed by
        param_names(STAGE_DECODER_MLP_NLL_BWD)); `pi.*` gets no gradient"""
        return self._mlp_decoder_backward(data, local_embed, global_embed, out, nll_eps=float(eps))

    def _mlp_decoder_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                              nll_eps: Optional[float]) -> Dict[str, object]:
        """shared body of mlp_decoder_l2_backward / mlp_decoder_nll_backward (`nll_eps` None: L2)"""
        m = self.module
        if nll_eps is not None and not getattr(m, "uncertain", True):
            raise _lib.TrajsdeError("LaplaceNLLLoss needs the decoder's scale head: `uncertain: False` has none "
                                    "(dec_hivt_nusargo_grid.py:31, losses/laplace_nll_loss.py:28 chunks loc | scale out of four channels)")
        dev = local_embed.device
        K, T, N = int(m.num_modes), int(m.future_steps), local_embed.shape[0]
        y, mask = self._targets_and_mask(data, out, N, T, "rotated targets")
        L = _lib.lib()
        stage = _lib.STAGE_DECODER_MLP_BWD if nll_eps is None else _lib.STAGE_DECODER_MLP_NLL_BWD
        names, grads, arr, d_local, d_global = self._backward_outputs(stage, N, K, dev)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        best = torch.empty(N, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            head = (N, K, T, self.blob(stage).data_ptr(), local_embed.contiguous().data_ptr(), global_embed.contiguous().data_ptr(),
                    _loc4(out).data_ptr(), y.data_ptr(), mask.data_ptr())
            tail = (loss.data_ptr(), best.data_ptr(), arr, len(names), d_local.data_ptr(), d_global.data_ptr(), _stream())
            if nll_eps is None:
                ws_bytes = L.trajsde_mlp_decoder_backward_ws_bytes(N)
                ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
                _lib.check(L.trajsde_mlp_decoder_l2_backward(*head, ws.data_ptr(), ws_bytes, *tail), "trajsde_mlp_decoder_l2_backward")
            else:
                ws_bytes = L.trajsde_mlp_decoder_nll_backward_ws_bytes(N)
                ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
                _lib.check(L.trajsde_mlp_decoder_nll_backward(*head, float(nll_eps), float(m.min_scale), ws.data_ptr(), ws_bytes, *tail),
                           "trajsde_mlp_decoder_nll_backward")
        return {"loss": loss[0], "best_mode": best, "grads": grads, "d_local_embed": d_local, "d_global_embed": d_global}

    def mlp_decoder_cotangent_backward(self, data, local_embed: torch.Tensor, global_embed: torch.Tensor, out: Dict[str, torch.Tensor],
                                       d_loc: Optional[torch.Tensor], d_pi: Optional[torch.Tensor]) -> Dict[str, object]:
        """Vector-Jacobian product of MLPDecoder.forward (dec_hivt_nusargo_grid.py:47-63) from caller-supplied cotangents: `d_loc` =
        dL/dloc [K,N,T,4] and `d_pi` = dL/dpi [N,K] of ANY loss over all K modes; None is zeros.  `out` = mlp_decoder_forward(...).
        All K * N rows are differentiated and so is the three-layer pi head.  Returns {"grads": {param name: tensor} keyed by
        param_names(STAGE_DECODER_MLP_COT_BWD) -- `scale.*` and `pi.*` included --, "d_local_embed", "d_global_embed"}."""
        m = self.module
        if not getattr(m, "uncertain", True):
            raise _lib.TrajsdeError("mlp_decoder_cotangent_backward needs the decoder's scale head: `uncertain: False` has none "
                                    "(dec_hivt_nusargo_grid.py:31)")
        _require_gpu(local_embed, "local_embed")
        dev = local_embed.device
        K, T, N = int(m.num_modes), int(m.future_steps), local_embed.shape[0]
        if tuple(local_embed.shape) != (N, D) or tuple(global_embed.shape) != (K, N, D):
            raise _lib.TrajsdeError(f"local_embed must be [{N},{D}] and global_embed [{K},{N},{D}], got {tuple(local_embed.shape)} and "
                                    f"{tuple(global_embed.shape)}")
        loc4 = _loc4(out)
        if tuple(loc4.shape) != (K, N, T, 4):
            raise _lib.TrajsdeError(f"out['loc'] must be [{K},{N},{T},4], got {tuple(loc4.shape)}")
        # (the one decoder backward that checks and casts the embeddings, a guard for callers that bring their own; the other three
        #  hand them to the kernels as given, float32 [N,64] and [K,N,64] as the stage forwards make them)
        local_c, global_c = local_embed.to(torch.float32).contiguous(), global_embed.to(torch.float32).contiguous()
        d_loc4, d_pi_c = self._cotangents(d_loc, d_pi, K, N, T, dev, allow_two_channels=False)
        L = _lib.lib()
        stage = _lib.STAGE_DECODER_MLP_COT_BWD
        names, grads, arr, d_local, d_global = self._backward_outputs(stage, N, K, dev)
        ws_bytes = self._checked_ws_bytes("trajsde_mlp_decoder_cotangent_backward_ws_bytes", N, K, T)
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            _lib.check(L.trajsde_mlp_decoder_cotangent_backward(
                N, K, T, self.blob(stage).data_ptr(), local_c.data_ptr(), global_c.data_ptr(), loc4.data_ptr(), float(m.min_scale),
                d_loc4.data_ptr(), d_pi_c.data_ptr(), ws.data_ptr(), ws_bytes, arr, len(names), d_local.data_ptr(), d_global.data_ptr(), _stream()),
                "trajsde_mlp_decoder_cotangent_backward")
        return {"grads": grads, "d_local_embed": d_local, "d_global_embed": d_global}


class GraphContext:
    """Device-side graph structures of one batch (CSR, compacted edge lists, segment pointers), built once per
    forward by the first stage that needs them and parked on the batch object for the next stage."""

    KEY = "_trajsde_graph"
    DEFAULT_RADIUS = 50.0
    _DEVICE_KEY_TOKENS = itertools.count(1)

    def __init__(self, data, radius: float, H: int, noise: Optional[NoiseSpec], fake_agents: bool = True,
                 exact: bool = True, sync_free_cap: Optional[int] = None) -> None:
        L = _lib.lib()
        self.fake_agents = fake_agents
        x = data["x"]
        _require_gpu(x, "data['x']")
        self.device = dev = x.device
        keep = self._keep = []

        def f32(t):
            t = t.to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        def u8(t):
            t = t.contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
            keep.append(t)
            return t.data_ptr()

        def i64(t):
            t = t.to(torch.int64).contiguous()
            keep.append(t)
            return t.data_ptr() if t.numel() else None

        N, Hx = x.shape[0], x.shape[1]
        if Hx != H:
            raise _lib.TrajsdeError(f"data['x'] has {Hx} history steps, the stage was built for {H}")
        if "rotate_mat" not in data or data["rotate_mat"] is None or data["rotate_mat"] is False:
            raise _lib.TrajsdeError("data['rotate_mat'] is missing: call the model's forward (MODEL:75-85) or runtime.rotate_inputs")
        self.rot = data["rotate_mat"].to(torch.float32).contiguous()
        ei, lai = data["edge_index"], data["lane_actor_index"]
        lp = data["lane_positions"]
        n_agents = data["agent_index"].numel() if fake_agents else 0      # A = 0: no fake rows (forward_ood, ENC:204-370)
        self.batch = _lib.Batch(N, n_agents, ei.shape[1], lp.shape[0], lai.shape[1], H,
                                data["positions"].shape[1], lp.shape[1] if lp.dim() > 1 else 0,
                                f32(x), f32(data["positions"]), u8(data["padding_mask"]), u8(data["bos_mask"]),
                                f32(data["rotate_angles"]), i64(ei), i64(data["agent_index"]) if fake_agents else None, i64(data["batch"]),
                                i64(data["source"]), f32(lp), f32(data["lane_paddings"]), i64(lai),
                                f32(data["lane_actor_vectors"]))
        if data["padding_mask"].shape[1] != data["positions"].shape[1]:
            raise _lib.TrajsdeError("padding_mask and positions must cover the same time slots")
        self.graph = _lib.Graph()
        noise = NoiseSpec.resolve(noise)
        z_fake = noise.z_fake if fake_agents else None
        if z_fake is not None and tuple(z_fake.shape) != (self.batch.A, H, 2):
            raise _lib.TrajsdeError(f"z_fake must be [{self.batch.A},{H},2]")
        cn = noise.c_noise(z_fake, noise.fake_row_ids)
        with torch.cuda.device(dev):
            ws_bytes = L.trajsde_graph_ws_bytes(C.byref(self.batch))
            if ws_bytes < 0:
                raise _lib.TrajsdeError("graph workspace query failed: " + L.trajsde_last_error().decode())
            self.ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
            # sync-free form: list lengths stay on the device, the E_* fields are bounds (int32 positions must hold them)
            b = self.batch
            # ... and the agent-agent list is allocated for the bound 2 H E (24 B per slot): past SYNC_FREE_MAX_BYTES the
            # one synchronisation is the better deal (8 scenes x 1024 agents would reserve 8 GB for 90 MB of edges)
            cap = SYNC_FREE_MAX_BYTES if sync_free_cap is None else int(sync_free_cap)
            if not exact and (2 * b.H * b.E >= 2 ** 31 - 2 or 24 * 2 * b.H * b.E > cap):
                exact = True
            prepare = L.trajsde_graph_prepare if exact else L.trajsde_graph_prepare_async
            _lib.check(prepare(C.byref(self.batch), self.rot.data_ptr(), float(radius), C.byref(cn),
                               self.ws.data_ptr(), ws_bytes, C.byref(self.graph), _stream()), "trajsde_graph_prepare")
            ews_bytes = L.trajsde_graph_edges_ws_bytes(C.byref(self.batch), C.byref(self.graph))
            self.edges_ws = torch.empty(ews_bytes, device=dev, dtype=torch.uint8)
            _lib.check(L.trajsde_graph_compact(C.byref(self.batch), self.rot.data_ptr(), self.ws.data_ptr(), ws_bytes,
                                               self.edges_ws.data_ptr(), ews_bytes, C.byref(self.graph), _stream()),
                       "trajsde_graph_compact")

    def _i32(self, buf: torch.Tensor, ptr: Optional[int], n: int) -> torch.Tensor:
        """int32 view of `n` entries at device address `ptr` inside the workspace tensor `buf`"""
        if not ptr or n <= 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        off = ptr - buf.data_ptr()
        assert 0 <= off and off + 4 * n <= buf.numel() and off % 4 == 0
        return buf[off:off + 4 * n].view(torch.int32)

    def true_counts(self) -> Dict[str, int]:
        """the list lengths (a host synchronisation when the graph was built sync-free)"""
        g = self.graph
        if g.exact:
            return {"E_aa": g.E_aa, "E_g": g.E_g, "E_la": g.E_la}
        st = getattr(self, "count_stream", None)
        if st is not None:                    # built on a side stream (prefetch_graph): read there -- a read on the current stream
            with torch.cuda.stream(st):       # would wait for everything queued on it, i.e. for the whole previous training step
                c = self._i32(self.ws, g.counts, 4).tolist()
        else:
            c = self._i32(self.ws, g.counts, 4).tolist()
        return {"E_aa": c[1], "E_g": c[2], "E_la": c[3]}

    def graph_path(self) -> str:
        """which way the actor CSR of this graph was built: "direct" -- the edge list was in dataset order (per scene
        permutations(range(n), 2), scenes ascending) and the CSR was written from the closed form -- or "general" (histogram,
        scatter, row sort).  Decided on the device; reading it is a host synchronisation, like true_counts()."""
        st = getattr(self, "count_stream", None)
        if st is not None:
            with torch.cuda.stream(st):
                c = self._i32(self.ws, self.graph.counts, 8).tolist()
        else:
            c = self._i32(self.ws, self.graph.counts, 8).tolist()
        return "direct" if c[6] == 1 else "general"

    def make_exact(self) -> "GraphContext":
        """turn a sync-free graph into an exact one in place: read the counts (synchronises) and store them in the E_* fields.
        The buffers keep their bound-sized allocation; every entry point accepts the graph afterwards."""
        g = self.graph
        if not g.exact:
            c = self.true_counts()
            assert c["E_aa"] <= g.E_aa and c["E_g"] <= g.E_g and c["E_la"] <= g.E_la, "edge-count bound violated"
            g.E_aa, g.E_g, g.E_la, g.exact = c["E_aa"], c["E_g"], c["E_la"], 1
        return self

    def edge_lists(self) -> Dict[str, torch.Tensor]:
        """the compacted lists as tensors (copies): what ENC:107-118, AGG:41 and ENC:198 leave of the input edge lists, in
        this build's canonical order (target-major, senders ascending) -- for edge-for-edge comparison with the oracle"""
        self.make_exact()
        g, b = self.graph, self.batch
        n_aa = b.H * g.Nt
        return {"aa_src": self._i32(self.edges_ws, g.aa_src, g.E_aa).clone(), "aa_dst": self._i32(self.edges_ws, g.aa_dst, g.E_aa).clone(),
                "aa_segptr": self._i32(self.ws, g.aa_segptr, n_aa + 1).clone(),
                "g_src": self._i32(self.edges_ws, g.g_src, g.E_g).clone(), "g_dst": self._i32(self.edges_ws, g.g_dst, g.E_g).clone(),
                "g_segptr": self._i32(self.ws, g.g_segptr, b.N + 1).clone(),
                "la_lane": self._i32(self.edges_ws, g.la_lane, g.E_la).clone(), "la_dst": self._i32(self.edges_ws, g.la_dst, g.E_la).clone(),
                "la_segptr": self._i32(self.ws, g.la_segptr, b.N + 1).clone()}

    @staticmethod
    def _input_stamp(data) -> tuple:
        """identity AND in-place version of every batch tensor the graph is derived from: an edited batch never reuses a
        stale graph, even under a repeated noise seed"""
        out = []
        for k in ("x", "positions", "padding_mask", "bos_mask", "rotate_angles", "edge_index", "agent_index", "batch", "source",
                  "lane_positions", "lane_paddings", "lane_actor_index", "lane_actor_vectors", "rotate_mat"):
            t = data[k] if k in data else None
            if not torch.is_tensor(t):
                out.append(None)
                continue
            # inference tensors (a batch moved to the device under torch.inference_mode(), as Lightning's validate / test loops
            # do) track no version counter -- reading it raises.  They are stamped by identity alone: the encoder rebuilds the
            # graph whenever the noise key changes, i.e. on every forward with fresh noise, and the later stages of the SAME
            # forward reuse it.
            ver = -1 if t.is_inference() else t._version
            out.append((t.data_ptr(), ver, tuple(t.shape)))
        return tuple(out)

    @classmethod
    def get(cls, data, radius: Optional[float], H: int, noise: Optional[NoiseSpec], fake_agents: bool = True,
            want_senders: bool = False, exact: Optional[bool] = True, sync_free_cap: Optional[int] = None) -> "GraphContext":
        """`exact`: True -- the caller's entry point needs the list lengths on the host (training, backward, captures of
        intermediates); False -- build sync-free if a build is needed; None -- take whatever the encoder left."""
        gc = data[cls.KEY] if cls.KEY in data else None
        if gc is not None and want_senders and not gc.graph.aa_src and gc.graph.E_aa > 0:
            gc = None                                                     # built without the sender ids: rebuild
        key = None
        if radius is not None and noise is not None:
            # a device-resident key (NoiseSpec.seed_dev) can change without the host seeing it, and the fake agents' rows are
            # drawn from it: such a graph is never reused across encoder calls (a fresh token per build request)
            dev_key = None if noise.seed_dev is None else next(cls._DEVICE_KEY_TOKENS)
            key = (float(radius), int(noise.seed), dev_key, id(noise.z_fake), id(noise.fake_row_ids), bool(fake_agents),
                   cls._input_stamp(data))
        elif gc is not None and getattr(gc, "build_key", None) is not None and gc.build_key[-1] != cls._input_stamp(data):
            gc = None                                                     # the batch was edited since the encoder built the graph
        if gc is None or (key is not None and getattr(gc, "build_key", None) != key):
            # the encoder (which owns the radius and the fake-agent noise) builds; the aggregator and the backward
            # entry points of the same step (same noise) reuse
            gc = cls(data, cls.DEFAULT_RADIUS if radius is None else radius, H, noise, fake_agents, exact=exact is not False,
                     sync_free_cap=sync_free_cap)
            gc.build_key = key
            data[cls.KEY] = gc
        if exact:
            gc.make_exact()
        return gc


# ---------------------------------------------------------------------------------------------------- one shape for any batch that fits
@dataclass(frozen=True)
class BatchCapacity:
    """The largest batch a set of CapacityBuffers takes: actors, scenes (= target agents), columns of `edge_index`, lane segments, columns
    of `lane_actor_index`.  The static buffers hold this plus a permanent reserve of one scene, two actors and one lane
    (`padded_sizes()`), so that pad edges always have inert endpoints -- also for a batch that fills the capacity.  Every scene
    slot a batch leaves empty is a pad scene of one pad actor (the number of fake agents is part of the static shape), hence the rule
    `N + (scenes - S) <= actors` of `fits()`."""
    actors: int
    scenes: int
    edges: int
    lanes: int
    lane_edges: int

    RESERVE_ACTORS, RESERVE_SCENES, RESERVE_LANES = 2, 1, 1

    def __post_init__(self) -> None:
        if self.actors < 1 or self.scenes < 1 or min(self.edges, self.lanes, self.lane_edges) < 0:
            raise ValueError(f"{self}: a capacity holds at least one actor and one scene, and no negative size")
        if self.actors < self.scenes:
            raise ValueError(f"{self}: every scene holds an actor -- fewer actors than scenes fit no batch")

    @staticmethod
    def sizes_of(batch) -> Dict[str, int]:
        """{actors, scenes, edges, lanes, lane_edges} of a batch, from shapes alone (any device, no synchronisation)"""
        return {"actors": int(batch["x"].shape[0]), "scenes": int(batch["agent_index"].numel()), "edges": int(batch["edge_index"].shape[1]),
                "lanes": int(batch["lane_positions"].shape[0]), "lane_edges": int(batch["lane_actor_index"].shape[1])}

    @classmethod
    def covering(cls, batches) -> "BatchCapacity":
        """the smallest capacity every one of `batches` (batch objects, or dicts as `sizes_of` returns them) fits: one host pass over sizes"""
        sizes = [b if isinstance(b, dict) else cls.sizes_of(b) for b in batches]
        if not sizes:
            raise ValueError("BatchCapacity.covering needs at least one batch")
        scenes = max(s["scenes"] for s in sizes)
        return cls(actors=max(s["actors"] + scenes - s["scenes"] for s in sizes), scenes=scenes, edges=max(s["edges"] for s in sizes),
                   lanes=max(s["lanes"] for s in sizes), lane_edges=max(s["lane_edges"] for s in sizes))

    def why_not(self, batch) -> Optional[str]:
        """None when the batch fits, else a message that names the first overflowing dimension"""
        s = batch if isinstance(batch, dict) else self.sizes_of(batch)
        if s["scenes"] < 1 or s["actors"] < 1:
            return "an empty batch (no scene or no actor)"
        if s["scenes"] > self.scenes:
            return f"scenes: {s['scenes']} exceed the capacity of {self.scenes}"
        if s["actors"] + (self.scenes - s["scenes"]) > self.actors:
            return (f"actors: {s['actors']} plus one for each of the {self.scenes - s['scenes']} pad scenes exceed the capacity of "
                    f"{self.actors}")
        for dim in ("edges", "lanes", "lane_edges"):
            if s[dim] > getattr(self, dim):
                return f"{dim}: {s[dim]} exceed the capacity of {getattr(self, dim)}"
        return None

    def fits(self, batch) -> bool:
        return self.why_not(batch) is None

    def padded_sizes(self) -> Tuple[int, int, int, int, int]:
        """(N, A, E, L, E_al) of the static buffers: the capacity plus the reserve"""
        return (self.actors + self.RESERVE_ACTORS, self.scenes + self.RESERVE_SCENES, self.edges, self.lanes + self.RESERVE_LANES,
                self.lane_edges)


PAD_FAR_RADII = 200.0          # a pad lane-actor vector is (200 r, 200 r) for local_radius r (csrc/pad.hip): the radius filter drops it


def pad_batch_host(batch, capacity: BatchCapacity, num_modes: int, local_radius: Optional[float] = None):
    """The torch twin of trajsde_batch_pad (include/trajsde_hip_capacity.h), on the tensors' own device (meant for the host: it is the
    launch's oracle and the input of the CPU oracle test): -> (the padded batch, {"fake_row_ids", "enc_row_ids", "dec_row_ids"}).
    Masks come out as bool, floats as float32, indices as int64, row ids as int32.  A batch of zero actors and zero scenes is
    accepted (the all-padding state CapacityBuffers start in)."""
    from trajsde_amd.data import TemporalData
    why = None if int(batch["x"].shape[0]) == 0 and int(batch["agent_index"].numel()) == 0 else capacity.why_not(batch)
    if why is not None:
        raise _lib.TrajsdeError(f"the batch does not fit the capacity -- {why}")
    radius = GraphContext.DEFAULT_RADIUS if local_radius is None else float(local_radius)
    far = PAD_FAR_RADII * radius if radius > 0 else 0.0
    Np, Ap, Ep, Lp, Eap = capacity.padded_sizes()
    x = batch["x"]
    dev = x.device
    N, S, K = int(x.shape[0]), int(batch["agent_index"].numel()), int(num_modes)
    E, L, Ea = int(batch["edge_index"].shape[1]), int(batch["lane_positions"].shape[0]), int(batch["lane_actor_index"].shape[1])
    pad_scenes = Ap - S
    base = N + pad_scenes - 1                                   # first actor of the permanent pad scene
    M = Np - base                                               # its actors: >= 2
    i64 = dict(dtype=torch.int64, device=dev)

    def rows(t, n, fill, dtype):
        t = t.to(dtype)
        out = torch.full((n,) + tuple(t.shape[1:]), fill, dtype=dtype, device=dev)
        out[:t.shape[0]] = t
        return out

    out = {"x": rows(x, Np, 0.0, torch.float32), "positions": rows(batch["positions"], Np, 0.0, torch.float32),
           "padding_mask": rows(batch["padding_mask"], Np, True, torch.bool), "bos_mask": rows(batch["bos_mask"], Np, False, torch.bool),
           "rotate_angles": rows(batch["rotate_angles"], Np, 0.0, torch.float32),
           "lane_positions": rows(batch["lane_positions"], Lp, 0.0, torch.float32),
           "lane_paddings": rows(batch["lane_paddings"], Lp, 0.0, torch.float32),
           "lane_actor_vectors": rows(batch["lane_actor_vectors"], Eap, far, torch.float32)}
    if batch.y is not None:
        out["y"] = rows(batch.y, Np, 0.0, torch.float32)
    j = torch.arange(Ep - E, **i64)
    d = j % M
    s = (d + 1 + (j // M) % (M - 1)) % M
    out["edge_index"] = torch.cat([batch["edge_index"].to(torch.int64), torch.stack([base + s, base + d])], dim=1)
    out["agent_index"] = torch.cat([batch["agent_index"].to(torch.int64).reshape(-1), N + torch.arange(pad_scenes, **i64)])
    out["batch"] = torch.cat([batch["batch"].to(torch.int64), S + torch.arange(Np - N, **i64).clamp(max=pad_scenes - 1)])
    out["source"] = torch.cat([batch["source"].to(torch.int64).reshape(-1), torch.zeros(pad_scenes, **i64)])
    j = torch.arange(Eap - Ea, **i64)
    out["lane_actor_index"] = torch.cat([batch["lane_actor_index"].to(torch.int64), torch.stack([torch.full_like(j, Lp - 1), base + j % M])], dim=1)
    out["num_nodes"] = Np
    i = torch.arange(Np + Ap, **i64)
    enc = torch.where(i < N, i, torch.where(i < Np, i + S, torch.where(i - Np < S, N + (i - Np), i)))
    n = torch.arange(Np, **i64)
    k = torch.arange(K, **i64)[:, None]
    dec = torch.where(n[None, :] < N, k * N + n[None, :], K * N + k * (Np - N) + (n[None, :] - N))
    ids = {"fake_row_ids": torch.arange(Ap, dtype=torch.int32, device=dev), "enc_row_ids": enc.to(torch.int32),
           "dec_row_ids": dec.reshape(-1).to(torch.int32)}
    return TemporalData(**out), ids


def _empty_batch(H: int, TT: int, lane_pts: int):
    """a batch of no actor and no scene: pad_batch_host of it is the all-padding state"""
    from trajsde_amd.data import TemporalData
    z = torch.zeros
    return TemporalData(x=z(0, H, 2), positions=z(0, TT, 2), padding_mask=z(0, TT, dtype=torch.bool), bos_mask=z(0, H, dtype=torch.bool),
                        rotate_angles=z(0), edge_index=z(2, 0, dtype=torch.int64), agent_index=z(0, dtype=torch.int64),
                        batch=z(0, dtype=torch.int64), source=z(0, dtype=torch.int64), lane_positions=z(0, lane_pts, 2),
                        lane_paddings=z(0, lane_pts), lane_actor_index=z(2, 0, dtype=torch.int64), lane_actor_vectors=z(0, 2),
                        y=z(0, TT - H, 2))


def _c_batch(data, n_agents: Optional[int] = None, keep: Optional[list] = None) -> "_lib.Batch":
    """the C struct over a batch's device tensors, in the dtypes the kernels read (float32 / bytes / int64: converted copies where a
    tensor has another, kept alive in `keep`)"""
    keep = [] if keep is None else keep

    def ptr(t, dtype):
        if dtype is torch.uint8:
            t = t.contiguous()
            t = t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)
        else:
            t = t.to(dtype).contiguous()
        keep.append(t)
        return t.data_ptr() if t.numel() else None

    f, u, i = torch.float32, torch.uint8, torch.int64
    lp, ei, lai = data["lane_positions"], data["edge_index"], data["lane_actor_index"]
    return _lib.Batch(data["x"].shape[0], data["agent_index"].numel() if n_agents is None else n_agents, ei.shape[1], lp.shape[0], lai.shape[1],
                      data["x"].shape[1], data["positions"].shape[1], lp.shape[1] if lp.dim() > 1 else 0,
                      ptr(data["x"], f), ptr(data["positions"], f), ptr(data["padding_mask"], u), ptr(data["bos_mask"], u),
                      ptr(data["rotate_angles"], f), ptr(ei, i), ptr(data["agent_index"], i), ptr(data["batch"], i), ptr(data["source"], i),
                      ptr(lp, f), ptr(data["lane_paddings"], f), ptr(lai, i), ptr(data["lane_actor_vectors"], f))


class CapacityBuffers:
    """Capacity-sized static batch tensors and row-id tables on a device, filled by ONE launch per batch (trajsde_batch_pad, csrc/pad.hip):

        buf = CapacityBuffers(BatchCapacity.covering(batches), num_modes=K, device=dev, time_slots=21 + F)
        buf.stage(batch)                                    # any batch that fits: same shapes, same addresses, inert padding
        out = model(buf.batch, noise=buf.noise(seed))       # real rows: model(batch, noise=NoiseSpec(seed=seed)), see pad_batch_host

    `buf.batch` keeps its tensors' shapes and addresses over every `stage()`; `buf.noise(seed)` keys the three noise streams by the
    row-id tables, so the real rows (`[:N]` of loc / pi / reg_mask, `[:S]` of diff_in / diff_out) draw the noise of the unpadded
    batch.  Every call overwrites every element of every tensor and table: a smaller batch after a larger one leaves nothing behind.
    Monte-Carlo decoding keys sample s by `row id + s * sample_stride`, and its default stride is K * N of the tensor it is handed --
    K * N_padded here, under which only sample 0 is the unpadded call's.  `buf.sample_stride` is K * N of the batch staged last (from
    its shape: no device read; None before the first `stage()`):
        out = model.predict_samples(buf.batch, R, noise=buf.noise(seed), sample_stride=buf.sample_stride)
    gives every sample of the unpadded `model.predict_samples(batch, R, noise=NoiseSpec(seed=seed))` on the real rows.  (The ids of the
    real rows of sample s >= 1 then coincide with ids of PAD rows of earlier samples, never with another real (row, sample).)
    Refused with a message: a host tensor or one on another device among the batch's, a batch that does not fit (`why_not`), other
    time slots or points per lane.
    The forward REBINDS `buf.batch.y` to its rotated copy (MODEL:83-84): `stage()` puts the static tensor back."""

    def __init__(self, capacity: BatchCapacity, num_modes: int, device, time_slots: int, history_steps: int = 21, lane_points: int = 10,
                 local_radius: Optional[float] = None) -> None:
        if not isinstance(capacity, BatchCapacity):
            raise TypeError("capacity must be a runtime.BatchCapacity")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TrajsdeError("CapacityBuffers must live on the GPU: the staging launch has no CPU implementation "
                                    "(runtime.pad_batch_host is its torch twin)")
        if self.device.index is None:                     # ("cuda": the current device, spelled out -- stage() compares devices)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.num_modes = capacity, int(num_modes)
        self.H, self.TT, self.lane_pts = int(history_steps), int(time_slots), int(lane_points)
        self.F = self.TT - self.H
        if self.F < 1:
            raise _lib.TrajsdeError(f"CapacityBuffers: time_slots {self.TT} leave no future step behind the {self.H} history steps")
        self.radius = GraphContext.DEFAULT_RADIUS if local_radius is None else float(local_radius)
        # the all-padding state (the host twin's, copied over once)
        empty, ids = pad_batch_host(_empty_batch(self.H, self.TT, self.lane_pts), capacity, self.num_modes, self.radius)
        self.batch = empty.to(self.device)
        self._y = self.batch.y
        self.ids = {k: v.to(self.device) for k, v in ids.items()}
        self.sample_stride: Optional[int] = None          # K * N of the batch staged last (predict_samples' sample_stride)
        keep = []
        self._dst = _c_batch(self.batch, keep=keep)
        # the launch writes through these addresses on every stage(): each must be the static tensor's own, not a converted copy's
        held = {t.data_ptr() for t in keep if t.numel()}
        own = {v.data_ptr() for v in self.batch.as_dict().values() if torch.is_tensor(v) and v.numel()}
        if not held <= own:
            raise _lib.TrajsdeError("CapacityBuffers: a static tensor is not in the dtype / layout the launch writes (internal error)")

    def why_not(self, batch) -> Optional[str]:
        """None when `batch` can be staged, else a message that names what does not fit"""
        why = self.capacity.why_not(batch)
        if why is None and int(batch["x"].shape[1]) != self.H:
            why = f"history steps: {int(batch['x'].shape[1])}, the buffers have {self.H}"
        if why is None and int(batch["positions"].shape[1]) != self.TT:
            why = f"time slots of positions / padding_mask: {int(batch['positions'].shape[1])}, the buffers have {self.TT}"
        lp = batch["lane_positions"]
        if why is None and lp.shape[0] > 0 and int(lp.shape[1]) != self.lane_pts:
            why = f"points per lane: {int(lp.shape[1])}, the buffers have {self.lane_pts}"
        y = batch.y
        if why is None and y is not None and tuple(y.shape) != (int(batch["x"].shape[0]), self.F, 2):
            why = f"targets y {tuple(y.shape)}, the buffers have [N,{self.F},2]"
        return why

    def fits(self, batch) -> bool:
        return self.why_not(batch) is None

    def stage(self, batch) -> None:
        """`batch` (device tensors) into the static tensors and the row-id tables: one launch on the current stream"""
        for k in ("x", "positions", "padding_mask", "bos_mask", "rotate_angles", "edge_index", "agent_index", "batch", "source",
                  "lane_positions", "lane_paddings", "lane_actor_index", "lane_actor_vectors", "y"):
            t = batch[k]
            if t is None:                                 # (only `y` may be absent)
                continue
            _require_gpu(t, f"data['{k}']")
            if t.device != self.device:
                raise _lib.TrajsdeError(f"data['{k}'] lives on {t.device}, these buffers on {self.device}: the staging launch reads and "
                                        "writes one device")
        why = self.why_not(batch)
        if why is not None:
            raise _lib.TrajsdeError(f"the batch does not fit these buffers ({self.capacity}) -- {why}")
        keep = []
        src = _c_batch(batch, keep=keep)
        src.lane_pts = self.lane_pts                      # (a batch without lanes: an empty lane tensor of any second dimension)
        y = batch.y
        if y is not None:
            y = y.to(torch.float32).contiguous()
        ids = self.ids
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().trajsde_batch_pad(C.byref(src), _ptr(y), self.F, C.byref(self._dst), self._y.data_ptr(), self.num_modes,
                                                    self.radius, ids["fake_row_ids"].data_ptr(), ids["enc_row_ids"].data_ptr(),
                                                    ids["dec_row_ids"].data_ptr(), _stream()), "trajsde_batch_pad")
        self.batch.y = self._y
        self.sample_stride = self.num_modes * int(batch["x"].shape[0])
        if GraphContext.KEY in self.batch:                # the launch writes in place: no version counter moves, so the graph a forward
            del self.batch[GraphContext.KEY]              # parked on the buffers would pass for current -- the next forward builds its own

    def noise(self, seed: int) -> NoiseSpec:
        """NoiseSpec(seed) keyed by the row-id tables of the batch staged last"""
        return NoiseSpec(seed=int(seed), fake_row_ids=self.ids["fake_row_ids"], enc_row_ids=self.ids["enc_row_ids"],
                         dec_row_ids=self.ids["dec_row_ids"])
