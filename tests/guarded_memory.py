"""Red-zone arenas for the memory contract of include/trajsde_hip.h ("BORROWS its pointers", "writes only into caller-provided
buffers", workspace sizes from the *_ws_bytes queries): tests/test_gpu_memory_contract.py, self-test tests/test_guarded_memory_cpu.py.

An arena is ONE uint8 tensor laid out as  [lead guard | interior | tail guard].  Both guards are G bytes (G >= 64 KiB -- 256 rows of
64 fp32, the largest single tile store in csrc/ is 32 rows -- and a multiple of 512, so that the interior keeps the 512-byte alignment
torch's caching allocator gives; the Carver of csrc/common.hpp assumes a 256-byte-aligned base).  The tail guard starts at the exact
byte where the requested size ends.  Every stray access this harness can see therefore lands inside the arena's own allocation: the
tests that use it cannot fault the device.

  GuardedMemory.placed(tensor, fill)   an INPUT copied into an arena -> the interior view (same dtype and shape, contiguous).  The guards
                                       are filled in the tensor's own type with values that are legal for its role, so that an overread
                                       changes the result without sending a dependent load somewhere wild:
                                           float fields  NaN (fill "A") / 1e30 (fill "B")
                                           int64 index fields  0 / 1   (use them only in batches where 0 and 1 are valid ids)
                                           mask bytes  0 / 1
                                       check() also reports whether the interior changed (inputs are `const` in the ABI).
  with GuardedMemory(poison=...):      torch.empty / empty_like / zeros / zeros_like of DEVICE memory (what trajsde_amd/runtime.py
                                       allocates everything with) come out of arenas while the context is active.  `empty` interiors are
                                       pre-filled with the poison: "nan" (all bytes 0xFF: a NaN as fp32, bf16 and fp16 alike, and -1 -- not
                                       a wild offset -- should a kernel take it for an int32), "zero", or an int = seeded random bits;
                                       `zeros` interiors are zero.  CPU and pinned allocations, zero-byte requests, allocations with
                                       arguments other than sizes / dtype / device, and everything outside the context pass through.
                                       The object keeps every arena alive until it is dropped, so a workspace the runtime released
                                       before the stream was synchronised is still there to be checked (and is never handed out twice).
  GuardedMemory.check()                after torch.cuda.synchronize(): every guard byte of every arena against its fill (which arena,
                                       where it was allocated, at which offset), and every placed interior against its snapshot.

Limits of the method:
  - a write that jumps further than G past a buffer is not seen;
  - a stray read whose value is masked before use is not seen;
  - an overrun from one carved sub-buffer of a workspace into the next, INSIDE the workspace, is not seen by the guards, and the
    *_ws_bytes queries carry up to 1 KiB of deliberate slack at the end, so a workspace's tail guard is looser than an output's.  The
    poison runs cover part of this: a sub-buffer read before it is written shows up as NaN or as a difference between poisons.
"""
import traceback

import torch

GUARD_BYTES = 64 * 1024
CANARY = 0xC3                                  # guard byte of routed allocations (outputs, workspaces: nothing legal reads past them)
_ORIG = {name: getattr(torch, name) for name in ("empty", "empty_like", "zeros", "zeros_like")}   # torch's own, taken at import
FILLS = {"float": {"A": float("nan"), "B": 1e30}, "index": {"A": 0, "B": 1}, "mask": {"A": 0, "B": 1}}


def role_of(dtype):
    if dtype.is_floating_point:
        return "float"
    if dtype == torch.int64:
        return "index"
    if dtype in (torch.bool, torch.uint8):
        return "mask"
    raise TypeError(f"no guard fill defined for {dtype}")


class Arena:
    def __init__(self, mem, nbytes, guard, pattern, label, where, kind):
        self.mem, self.nbytes, self.guard, self.pattern = mem, int(nbytes), int(guard), pattern
        self.label, self.where, self.kind = label, where, kind
        self.snapshot = None                                       # placed inputs: the interior bytes as they were handed over

    @property
    def interior_start(self):
        return self.mem.data_ptr() + self.guard

    @property
    def interior_end(self):
        return self.interior_start + self.nbytes

    def interior(self):
        return self.mem[self.guard:self.guard + self.nbytes]

    def contains(self, ptr, nbytes=0):
        """`ptr` (and the `nbytes` after it) inside the interior; an empty interior owns its own start"""
        return self.interior_start <= ptr and ptr + nbytes <= self.interior_end

    def __repr__(self):
        return f"<arena {self.label!r} {self.kind} {self.nbytes} B, allocated at {self.where}>"


class Report:
    """what check() found: `hits` [(arena, "lead" | "tail", offset, bytes touched)] with `offset` counted from the interior's start
    (negative: lead guard) or, for the tail guard, from the interior's end; `changed` [(arena, first changed interior byte)]"""

    def __init__(self, hits, changed, n_arenas):
        self.hits, self.changed, self.n_arenas = hits, changed, n_arenas

    @property
    def ok(self):
        return not self.hits and not self.changed

    def __str__(self):
        lines = [f"{self.n_arenas} arenas checked"]
        for a, side, off, n in self.hits:
            at = f"interior_start{off:+d}" if side == "lead" else f"interior_end+{off}"
            lines.append(f"GUARD TOUCHED: {side} guard of {a!r}: first byte at {at}, {n} bytes differ")
        for a, off in self.changed:
            lines.append(f"INPUT CHANGED: {a!r}: first byte at interior_start+{off}")
        return "\n".join(lines)


def _caller():
    """file:line of the frame that asked for the memory (outside this module and outside torch)"""
    for fr in reversed(traceback.extract_stack()[:-2]):
        if fr.filename != __file__ and "/torch/" not in fr.filename.replace("\\", "/"):
            return f"{fr.filename.rsplit('/', 1)[-1]}:{fr.lineno} ({fr.name})"
    return "?"


class GuardedMemory:
    _active = None                                                   # one context at a time patches torch's factory functions

    def __init__(self, poison="nan", guard_bytes=GUARD_BYTES, route=("cuda",)):
        """`poison`: "nan", "zero" or an int seed (random bits); `route`: the device types whose allocations are routed while the
        context is active (("cpu",) lets the self-test exercise the routing without a GPU; pinned memory always passes through)"""
        if guard_bytes < 64 * 1024 or guard_bytes % 512:
            raise ValueError("guards are >= 64 KiB and a multiple of 512 bytes")
        if not (poison in ("nan", "zero") or isinstance(poison, int)):
            raise ValueError("poison is 'nan', 'zero' or an int seed")
        self.poison, self.guard, self.route = poison, int(guard_bytes), tuple(route)
        self.arenas, self.routed, self.passed = [], 0, 0
        self._orig, self._gens, self._expected = dict(_ORIG), {}, {}

    # ------------------------------------------------------------------------------------------------ arenas
    def _new_arena(self, nbytes, device, pattern, label, kind):
        """[guard | nbytes | guard] with both guards holding `pattern` (a uint8 tensor of one element's bytes) repeated"""
        G = self.guard
        mem = _ORIG["empty"](G + nbytes + G, dtype=torch.uint8, device=device)
        assert mem.device.type != "cuda" or mem.data_ptr() % 512 == 0, "the caching allocator hands out 512-byte-aligned blocks"
        k = pattern.numel()
        assert G % k == 0 and nbytes % k == 0
        pat = pattern.to(mem.device)
        mem[:G].view(-1, k).copy_(pat.expand(G // k, k))
        mem[G + nbytes:].view(-1, k).copy_(pat.expand(G // k, k))
        a = Arena(mem, nbytes, G, pat, label, _caller(), kind)
        self.arenas.append(a)
        return a

    def placed(self, tensor, fill="A", label=None, const=True):
        """copy an input into an arena whose guards hold fill "A" / "B" of the tensor's role -> the interior view; `const=False`: a
        buffer the entry point updates in place (its interior is not compared with a snapshot)"""
        role = role_of(tensor.dtype)
        src = tensor.contiguous()
        one = torch.tensor([FILLS[role][fill]], dtype=src.dtype)
        a = self._new_arena(src.numel() * src.element_size(), src.device, one.view(torch.uint8), label or f"input {tuple(src.shape)}", "placed")
        view = a.interior().view(src.dtype).view(src.shape)
        view.copy_(src)
        if const:
            a.snapshot = a.interior().clone()
        return view

    def _alloc(self, shape, dtype, device, zero):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * _ORIG["empty"]((), dtype=dtype).element_size()
        a = self._new_arena(nbytes, device, torch.tensor([CANARY], dtype=torch.uint8), f"{'zeros' if zero else 'empty'}{shape} {dtype}", "alloc")
        inner = a.interior()
        if zero or self.poison == "zero":
            inner.zero_()
        elif self.poison == "nan":
            inner.fill_(0xFF)
        else:
            key = str(inner.device)
            if key not in self._gens:
                self._gens[key] = torch.Generator(device=inner.device).manual_seed(int(self.poison))
            inner.random_(0, 256, generator=self._gens[key])
        self.routed += 1
        return inner.view(dtype).view(shape)

    def _routes(self, device, kwargs, allowed):
        """route this request? -- a device of a routed type, no pinning, no argument this module does not model"""
        if device is None or torch.device(device).type not in self.route:
            return False
        if kwargs.get("pin_memory") or any(k not in allowed for k in kwargs):
            return False
        if kwargs.get("requires_grad") or kwargs.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format):
            return False
        return True

    def _factory(self, name, zero):
        orig = self._orig[name]

        def factory(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
            ok = self._routes(kw.get("device"), kw, ("dtype", "device", "requires_grad", "pin_memory", "memory_format")) and \
                all(isinstance(s, int) for s in shape) and len(shape) > 0
            if ok:
                n = 1
                for s in shape:
                    n *= int(s)
                ok = n > 0                                            # zero-byte requests keep their present behaviour
            if not ok:
                self.passed += 1
                return orig(*size, **kw)
            return self._alloc(shape, kw.get("dtype"), kw["device"], zero)
        return factory

    def _like(self, name, zero):
        orig = self._orig[name]

        def like(t, **kw):
            ok = torch.is_tensor(t) and t.numel() > 0 and t.is_contiguous() and not t.is_sparse and \
                self._routes(kw.get("device", t.device), kw, ("dtype", "device", "requires_grad", "pin_memory", "memory_format")) and \
                not (t.device.type == "cpu" and t.is_pinned())
            if not ok:
                self.passed += 1
                return orig(t, **kw)
            return self._alloc(t.shape, kw.get("dtype", t.dtype), kw.get("device", t.device), zero)
        return like

    def __enter__(self):
        if GuardedMemory._active is not None:
            raise RuntimeError("a GuardedMemory context is already active")
        GuardedMemory._active = self
        self._orig = dict(_ORIG)
        torch.empty, torch.zeros = self._factory("empty", False), self._factory("zeros", True)
        torch.empty_like, torch.zeros_like = self._like("empty_like", False), self._like("zeros_like", True)
        return self

    def __exit__(self, *exc):
        for name, fn in _ORIG.items():
            setattr(torch, name, fn)
        GuardedMemory._active = None
        return False

    # ------------------------------------------------------------------------------------------------ queries
    def arena_of(self, ptr, nbytes=0):
        """the arena whose interior holds [ptr, ptr + nbytes), or None"""
        for a in self.arenas:
            if a.contains(int(ptr), int(nbytes)):
                return a
        return None

    def owns(self, t):
        """a tensor (or a raw address) that lies inside one of this object's interiors"""
        if torch.is_tensor(t):
            return self.arena_of(t.data_ptr(), t.numel() * t.element_size()) is not None
        return t is not None and self.arena_of(t) is not None

    def check(self):
        """compare every guard with its fill and every placed interior with its snapshot (synchronise the device first)"""
        hits, changed = [], []
        for a in self.arenas:
            G, k = a.guard, a.pattern.numel()
            key = (str(a.mem.device), bytes(a.pattern.cpu().tolist()))
            want = self._expected.get(key)
            if want is None:
                want = self._expected[key] = a.pattern.repeat(G // k)
            for side, sl, base in (("lead", a.mem[:G], -G), ("tail", a.mem[G + a.nbytes:], 0)):
                bad = sl != want
                if bool(bad.any()):
                    idx = bad.nonzero()
                    hits.append((a, side, base + int(idx[0]), int(idx.numel())))
            if a.snapshot is not None and a.nbytes:
                bad = a.interior() != a.snapshot
                if bool(bad.any()):
                    changed.append((a, int(bad.nonzero()[0])))
        return Report(hits, changed, len(self.arenas))
