"""Scratch memory with chosen contents: the harness of the workspace contract (include/diffab_hip.h, "Workspaces and tapes").

Every hot-path entry works in memory it does not initialise itself: workspaces and tapes from _hip.workspace (a torch.empty), outputs
from torch.empty / torch.empty_like.  What those hold on entry is whatever the caching allocator had there - in a test process usually
zeros, or the previous call's buffer of the same size.  `poisoned(fill)` decides it instead, for its duration:

  - _hip.workspace returns the interior of a larger uint8 buffer with a GUARD-byte guard of 0xA5 in front and behind (GUARD = 4096 keeps
    the 256-byte alignment the library asks for); the interior holds `fill`.  Every base buffer lives until exit; check() synchronises
    and asserts that every guard byte still is 0xA5, naming the request's size and the offset of the first damaged byte relative to the
    interior (negative: in front of it).  Exit calls check() unless an exception is already on its way.
  - torch.empty and torch.empty_like call the original and then overwrite the bytes of a tensor on the target device with `fill`.
    Tensors on another device (CPU tensors when the target is a GPU, meta tensors), out= forms and non-strided layouts pass untouched.

Fills: "zero" (all zero bytes), "ff" (0xFF: NaN as f32 / f16, -1 as an integer, true as a mask byte), "random" (seeded random bytes
generated on the device: huge, denormal, Inf and NaN floats, arbitrary plan words) and "keep".  Under "keep" a new workspace starts as
zeros (what a fresh allocation usually holds) and is never refilled; a later request is served from the front of the smallest kept
buffer that is large enough and that nobody holds any more - the same buffer again for a size seen before - so a call finds exactly
what the previous one left: what the caching allocator does by accident, done on purpose.  (A smaller request's rear guard is the
larger buffer's; overruns are the other fills' business.)  torch.empty is left alone under "keep": the caller still holds the earlier
calls' outputs.  Whether somebody still holds a buffer (a tape saved for backward is held without any Python name) is read from the
storage's use count, torch._C._storage_Use_Count - a private API, so every new kept buffer checks that a view raises the count by one
and dropping it lowers it again, and raises RuntimeError otherwise; test_scratch_poison_host.py pins the same.

Not a test module and not a conftest.  Importing it loads no library and touches no device; `device` lets the logic run on CPU tensors
(tests/test_scratch_poison_host.py).  It does not mix with graph capture (the fills are launches of their own).
"""
import torch

from diffab_pytorch import _hip

GUARD = 4096
GUARD_BYTE = 0xA5
FILL_BYTE = {"zero": 0x00, "ff": 0xFF}
FILLS = ("zero", "ff", "random", "keep")


class GuardDamaged(AssertionError):
    pass


def raw_bytes(t):
    """The whole storage of `t` as a flat uint8 tensor (a view: writes land in t)."""
    return torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def _holders(base):
    return torch._C._storage_Use_Count(base.untyped_storage()._cdata)


class poisoned:
    def __init__(self, fill, seed=0, device=None):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, not {fill!r}")
        self.fill, self.seed = fill, seed
        self._device = None if device is None else torch.device(device)
        self.bases = []  # [base, requested bytes (the largest, under "keep"), holders when nobody has a view of it]
        self._saved = None
        self._gen = None

    # ------------------------------------------------------------------ the fills
    @property
    def device(self):
        if self._device is None:
            self._device = _hip.device()  # the current GPU, asked for at the first use
        return self._device

    def _targets(self, t):
        return isinstance(t, torch.Tensor) and t.layout == torch.strided and t.device.type == self.device.type

    def _fill_bytes(self, u8, fill):
        if u8.numel() == 0:
            return
        if fill == "random":
            if self._gen is None:
                self._gen = torch.Generator(device=u8.device).manual_seed(self.seed)
            for lo in range(0, u8.numel(), 1 << 28):  # (bounded transient memory for a tape of gigabytes)
                part = u8[lo:lo + (1 << 28)]
                part.copy_(self._saved["randint"](0, 256, (part.numel(),), dtype=torch.uint8, device=u8.device, generator=self._gen))
        else:
            u8.fill_(FILL_BYTE[fill])

    def _poison(self, t):
        if self.fill != "keep" and self._targets(t):
            self._fill_bytes(raw_bytes(t), self.fill)
        return t

    # ------------------------------------------------------------------ the three replaced names
    def _workspace(self, nbytes):
        n = max(int(nbytes), 256)
        if self.fill == "keep":
            free = [b for b in self.bases if b[1] >= n and _holders(b[0]) == b[2]]
            if free:
                return min(free, key=lambda b: b[1])[0][GUARD:GUARD + n]
        base = self._saved["empty"](n + 2 * GUARD, dtype=torch.uint8, device=self.device)
        base[:GUARD] = GUARD_BYTE
        base[GUARD + n:] = GUARD_BYTE
        self._fill_bytes(base[GUARD:GUARD + n], "zero" if self.fill == "keep" else self.fill)
        idle = _holders(base)
        if self.fill == "keep":  # the count is a private torch API: a torch whose holders count differently must not pass silently
            view = base[GUARD:GUARD + n]
            held = _holders(base)
            del view
            if held != idle + 1 or _holders(base) != idle:
                raise RuntimeError(f"torch._C._storage_Use_Count no longer counts one holder per view ({idle}, {held}, {_holders(base)}): "
                                   '"keep" cannot tell a free buffer from a held one')
        self.bases.append([base, n, idle])
        return base[GUARD:GUARD + n]

    def _empty(self, *args, **kw):
        t = self._saved["empty"](*args, **kw)
        return t if kw.get("out") is not None else self._poison(t)

    def _empty_like(self, *args, **kw):
        return self._poison(self._saved["empty_like"](*args, **kw))

    # ------------------------------------------------------------------ guards
    def check(self):
        if self.bases and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for base, n, _ in self.bases:
            for lo, part in ((-GUARD, base[:GUARD]), (n, base[GUARD + n:])):
                bad = (part != GUARD_BYTE).nonzero()
                if bad.numel():
                    first = int(bad[0])
                    raise GuardDamaged(f"a workspace of {n} bytes was written out of bounds: first damaged guard byte at offset "
                                       f"{lo + first} from its start ({int(bad.numel())} damaged bytes on that side, "
                                       f"value 0x{int(part[first]):02x})")

    def __enter__(self):
        self._saved = {"workspace": _hip.workspace, "empty": torch.empty, "empty_like": torch.empty_like, "randint": torch.randint}
        _hip.workspace, torch.empty, torch.empty_like = self._workspace, self._empty, self._empty_like
        return self

    def __exit__(self, exc_type, exc, tb):
        _hip.workspace, torch.empty, torch.empty_like = (self._saved[k] for k in ("workspace", "empty", "empty_like"))
        try:
            if exc_type is None:
                self.check()
        finally:
            self.bases.clear()
        return False
