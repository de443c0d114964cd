"""Parameter containers whose state_dict keys equal the reference's.

The stage modules own plain nn.Parameters -- the optimiser and checkpoints see exactly the names a
reference checkpoint has -- but no nn.Linear/LayerNorm *compute* modules: all arithmetic happens in
the HIP kernels, which read packed copies of these tensors.  `ParamTree` registers parameters under
dotted paths by creating nested anonymous containers ("a.b.0.weight" -> self.a.b.0.weight).

Initial values follow the reference's distributions (models/utils/util.py:94-159 init_weights:
xavier-uniform Linear weights, zero biases, LayerNorm ones/zeros -- the GRU unit included: its own N(0, 0.1) of
models/utils/ode_utils.py:211-215 is overwritten by the encoder's closing `self.apply(init_weights)`, ENC:49 then ENC:64;
N(0, 0.02) for tokens / hidden vectors).  tests/test_init_golden.py holds every family to moments taken from freshly
constructed reference models (oracle/make_golden_init.py).
"""
import math
from typing import Dict, Iterator, Optional, Tuple

import torch
import torch.nn as nn


class _Node(nn.Module):
    """Anonymous container; exists only to shape state_dict key names."""


class ParamTree(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self._gen: Optional[torch.Generator] = None

    def set_init_seed(self, seed: Optional[int]) -> None:
        """Initialise from a private CPU generator (reproducible, independent of the global RNG state;
        golden fixtures store only this seed).  None -> use the global RNG like the reference does."""
        self._gen = None if seed is None else torch.Generator().manual_seed(int(seed))

    # -- registration ---------------------------------------------------------------------------
    def _leaf_parent(self, path: str) -> Tuple[nn.Module, str]:
        parts = path.split(".")
        mod: nn.Module = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        return mod, parts[-1]

    def add_param(self, path: str, value: torch.Tensor, requires_grad: bool = True) -> nn.Parameter:
        mod, leaf = self._leaf_parent(path)
        p = nn.Parameter(value, requires_grad=requires_grad)
        mod.register_parameter(leaf, p)
        self.__dict__.pop("_stamp_slots", None)
        self.__dict__.pop("_p_slots", None)
        return p

    def absent(self, path: str, shape) -> None:
        """A tensor the reference's module does NOT have under this configuration (e.g. the decoder's `scale` head with
        `uncertain: False`, DEC:56 / dec_hivt_nusargo_grid.py:31) but the weight packer's recipe names: a zero stand-in held as a
        NON-persistent buffer -- it follows `.to()`, is in neither `state_dict()` nor `parameters()`, and `p(path)` resolves to it."""
        name = "_absent_" + path.replace(".", "_")
        self.register_buffer(name, torch.zeros(shape), persistent=False)
        self.__dict__.setdefault("_absent_paths", {})[path] = name
        self.__dict__.pop("_p_slots", None)

    def absent_head(self, path: str, in_f: int, d: int, out_f: int) -> None:
        for leaf, shape in ((".0.weight", (d, in_f)), (".0.bias", (d,)), (".1.weight", (d,)), (".1.bias", (d,)),
                            (".3.weight", (out_f, d)), (".3.bias", (out_f,))):
            self.absent(path + leaf, shape)

    def p(self, path: str) -> nn.Parameter:
        slots = self.__dict__.get("_p_slots")                               # path -> (container dict, leaf): survives re-assignment
        if slots is None:
            slots = self.__dict__["_p_slots"] = {}
        hit = slots.get(path)
        if hit is None:
            absent = self.__dict__.get("_absent_paths", {})
            if path in absent:
                hit = slots[path] = (self._buffers, absent[path])
            else:
                mod: nn.Module = self
                parts = path.split(".")
                for q in parts[:-1]:
                    mod = mod._modules[q]
                hit = slots[path] = (mod._parameters, parts[-1])
        return hit[0][hit[1]]

    # -- initialisers ---------------------------------------------------------------------------
    def _uniform(self, shape, bound):
        return (torch.rand(shape, generator=self._gen) * 2 - 1) * bound

    def _normal(self, shape, std):
        return torch.randn(shape, generator=self._gen) * std

    def linear(self, path: str, out_f: int, in_f: int, init: str = "xavier") -> None:
        if init == "xavier":
            w = self._uniform((out_f, in_f), math.sqrt(6.0 / (in_f + out_f)))
        elif init == "normal0.1":
            w = self._normal((out_f, in_f), 0.1)
        else:
            raise ValueError(init)
        self.add_param(path + ".weight", w)
        self.add_param(path + ".bias", torch.zeros(out_f))

    def layernorm(self, path: str, dim: int) -> None:
        self.add_param(path + ".weight", torch.ones(dim))
        self.add_param(path + ".bias", torch.zeros(dim))

    def token(self, path: str, *shape: int) -> None:
        self.add_param(path, self._normal(shape, 0.02))

    def constant(self, path: str, value: float) -> None:
        self.add_param(path, torch.tensor([[float(value)]]), requires_grad=False)

    # -- composite blocks shared by the stages ------------------------------------------------------
    def single_input_embedding(self, path: str, in_c: int, d: int) -> None:
        """keys of models/utils/embedding.py:22-40"""
        self.linear(f"{path}.embed.0", d, in_c)
        self.layernorm(f"{path}.embed.1", d)
        self.linear(f"{path}.embed.3", d, d)
        self.layernorm(f"{path}.embed.4", d)
        self.linear(f"{path}.embed.6", d, d)
        self.layernorm(f"{path}.embed.7", d)

    def multiple_input_embedding(self, path: str, in_cs, d: int) -> None:
        """keys of models/utils/embedding.py:43-70"""
        for i, c in enumerate(in_cs):
            self.linear(f"{path}.module_list.{i}.0", d, c)
            self.layernorm(f"{path}.module_list.{i}.1", d)
            self.linear(f"{path}.module_list.{i}.3", d, d)
        self.layernorm(f"{path}.aggr_embed.0", d)
        self.linear(f"{path}.aggr_embed.2", d, d)
        self.layernorm(f"{path}.aggr_embed.3", d)

    def attention_block(self, path: str, d: int, qkv=("lin_q", "lin_k", "lin_v")) -> None:
        """projection / gate / FFN parameters common to AAEncoder, ALEncoder, GlobalInteractorLayer."""
        for name in (*qkv, "lin_self", "lin_ih", "lin_hh", "out_proj"):
            self.linear(f"{path}.{name}", d, d)
        self.layernorm(f"{path}.norm1", d)
        self.layernorm(f"{path}.norm2", d)
        self.linear(f"{path}.mlp.0", 4 * d, d)
        self.linear(f"{path}.mlp.3", d, 4 * d)

    def sde_nets(self, path: str, d: int, g_names) -> None:
        """drift f (66-64-64-64), diffusion nets (66-64-64-1) and the frozen prior constants."""
        self.linear(f"{path}.f_func.net.0", d, d + 2)
        self.linear(f"{path}.f_func.net.2", d, d)
        self.linear(f"{path}.f_func.net.4", d, d)
        for g in g_names:
            self.linear(f"{path}.{g}.net.0", d, d + 2)
            self.linear(f"{path}.{g}.net.2", d, d)
            self.linear(f"{path}.{g}.net.4", 1, d)
        self.constant(f"{path}.h_func.theta", 1.0)
        self.constant(f"{path}.h_func.mu", 0.0)

    def head(self, path: str, in_f: int, d: int, out_f: int) -> None:
        self.linear(f"{path}.0", d, in_f)
        self.layernorm(f"{path}.1", d)
        self.linear(f"{path}.3", out_f, d)

    # -- bookkeeping used by the weight packers -------------------------------------------------
    def touch(self) -> None:
        """Say that parameter storage was modified through an alias the version counters do not see (driver.FlatTraining
        updates every parameter through one flat tensor they are slices of): the next forward re-packs the weight images."""
        self.__dict__["_touched"] = self.__dict__.get("_touched", 0) + 1

    def version_stamp(self) -> int:
        """Changes whenever any parameter is modified in place or re-assigned (optimizer step, load_state_dict, .to(), an in-place op
        on the parameter under no_grad).  A write through `p.data` (or any other alias, such as a flat tensor the parameters are
        views of) does NOT bump the parameter's `_version`: after one, call touch(), or the kernels keep the stale weight images.
        Called once per stage per forward, so it walks a cached list of (container dict, leaf name) slots instead of
        nn.Module.parameters() (0.2 ms of Python per call on this tree); the slots survive re-assignment of a leaf."""
        slots = self.__dict__.get("_stamp_slots")
        if slots is None:
            slots = [(mod._parameters, leaf) for mod in self.modules() for leaf in mod._parameters]
            self.__dict__["_stamp_slots"] = slots
        s = 0
        for d, leaf in slots:
            p = d[leaf]
            s = (s * 1000003 + p._version + (p.data_ptr() & 0xFFFF)) & 0xFFFFFFFFFFFF
        self.__dict__["_walk_stamp"] = s                      # versions and addresses alone (runtime.StageRuntime keys its pointer tables by it)
        return (s * 1000003 + self.__dict__.get("_touched", 0)) & 0xFFFFFFFFFFFF

    def walk_stamp(self) -> int:
        """the part of the last version_stamp() that does not move on touch(): same value = same tensors at the same addresses"""
        return self.__dict__.get("_walk_stamp", -1)
