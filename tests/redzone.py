"""Guard-banded allocations for tests: every tensor the Python layer allocates while ``redzone(device, fill)`` is open is carved out of a
larger uint8 block whose every byte holds ``fill``:

    [ GUARD bytes of fill | the request, ending on its exact last byte | GUARD bytes of fill ]

so that a store before the start or past the end of an output or workspace lands in a guard that ``check()`` reads back, a load outside an
input meets ``fill`` (0xFF: NaN in fp32 / fp16 / bf16, -1 in the integer types) instead of allocator slack that happens to hold zeros, and an
element that is never written keeps ``fill`` instead of whatever the caching allocator handed back.  A row is run under 0x00 (the state the
suite sees anyway) and then under 0xFF; a kernel that respects the contract in DESIGN.md ("Memory contract") leaves every guard byte alone,
leaves its inputs alone, and gives the same bits both times.

A plain helper module: no fixture, no plugin, and nothing is patched outside the ``with`` block.
"""
import contextlib
from collections import namedtuple

import torch

GUARD = 4096                 # a multiple of the allocator's 512-byte rounding: the interior starts as aligned as the block does
FILLS = (0x00, 0xFF)         # in this order: the 0x00 run is the state the rest of the suite sees

_FACTORIES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like")          # torch.<name>
_METHODS = ("new_empty", "new_zeros", "new_full", "new_ones")                          # torch.Tensor.<name>
_LIKE = ("empty_like", "zeros_like")
_MISSING = object()

Violation = namedtuple("Violation", "kind ordinal name shape dtype side offset count")
Violation.__str__ = lambda v: (
    f"{v.kind}: allocation #{v.ordinal}{'' if v.name is None else ' (' + v.name + ')'} {tuple(v.shape)} {v.dtype}, {v.side}: "
    f"{v.count} byte(s) changed, the first at offset {v.offset}")

_Block = namedtuple("_Block", "ordinal name base nbytes shape dtype clone tensor")


def _norm(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _extent(meta):
    """Bytes from the first to one past the last element of a strided tensor."""
    if meta.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(meta.shape, meta.stride())) + 1) * meta.element_size()


class Redzone:
    def __init__(self, device, fill, originals):
        assert 0 <= fill <= 0xFF
        self.device, self.fill, self._orig, self.blocks = _norm(device), fill, originals, []

    # ---- allocation ----
    def _carve(self, meta, name=None, keep_clone_of=None):
        """A tensor of ``meta``'s dtype, shape and strides whose storage is flush against a guard on both sides."""
        nbytes = _extent(meta)
        base = self._orig["empty"](2 * GUARD + nbytes, dtype=torch.uint8, device=self.device)
        base.fill_(self.fill)
        t = base[GUARD:GUARD + nbytes].view(meta.dtype).as_strided(tuple(meta.shape), tuple(meta.stride()))
        clone = None
        if keep_clone_of is not None:
            t.copy_(keep_clone_of)
            clone = base[GUARD:GUARD + nbytes].clone()
        self.blocks.append(_Block(len(self.blocks), name, base, nbytes, tuple(meta.shape), meta.dtype, clone, t))
        return t

    def place(self, t, name=None):
        """Copy an input tensor (from any device) into a carved block of the same dtype, shape and strides; a private clone is kept and
        ``check()`` reports the input if it no longer equals it."""
        meta = self._orig["empty_like"](t.detach(), device="meta")
        if _extent(meta) != meta.numel() * meta.element_size():        # not dense: place its contiguous form
            meta = self._orig["empty"](tuple(t.shape), dtype=t.dtype, device="meta")
        return self._carve(meta, name=name, keep_clone_of=t.detach())

    def place_module(self, module):
        """A deep copy of a (CPU) module whose every parameter and buffer is a placed input: packs built from it inside the block read weights that
        end flush against a guard, and their own planes are carved."""
        import copy
        if module is None:
            return None
        module = copy.deepcopy(module)
        for name, t in list(module.named_parameters()) + list(module.named_buffers()):
            t.data = self.place(t.data, name=name)
        return module

    def owns(self, t):
        """Is ``t`` (or the tensor it is a view of) one of this context's carved allocations?"""
        ptr = t.untyped_storage().data_ptr()
        return any(b.base.untyped_storage().data_ptr() == ptr for b in self.blocks)

    # ---- the check ----
    def check(self, written=()):
        """Violations after the work queued so far: guard bytes that no longer hold ``fill``, and placed inputs that changed (``written``: placed
        tensors, or their names, that the op documents as written in place).  One flag per block is reduced on the device and copied in one go;
        only blocks whose flag is set are looked at byte by byte."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self.blocks:
            return []
        exempt_names = {w for w in written if isinstance(w, str)}
        exempt_ids = {id(w) for w in written if not isinstance(w, str)}
        probes = []                                                     # (block, side, changed-bytes mask thunk)
        for b in self.blocks:
            probes.append((b, "guard before the start", lambda b=b: b.base[:GUARD] != self.fill))
            probes.append((b, "guard past the end", lambda b=b: b.base[GUARD + b.nbytes:] != self.fill))
            if b.clone is not None and b.name not in exempt_names and id(b.tensor) not in exempt_ids:
                probes.append((b, "interior", lambda b=b: b.base[GUARD:GUARD + b.nbytes] != b.clone))
        flags = torch.stack([mask().any() for _, _, mask in probes]).cpu().tolist()
        out = []
        for (b, side, mask), bad in zip(probes, flags):
            if bad:
                where = mask().nonzero().flatten()
                out.append(Violation("input changed" if side == "interior" else "guard byte changed", b.ordinal, b.name, b.shape, b.dtype,
                                     side, int(where[0]), int(where.numel())))
        return out

    # ---- the redirect ----
    def _redirect(self, name, original, like):
        def allocate(*args, **kwargs):
            device = kwargs.get("device")
            if device is None:
                device = (args[0] if args else kwargs["input"]).device if like else torch.get_default_device()
            if (_norm(device) != self.device or kwargs.get("pin_memory") or kwargs.get("out") is not None
                    or kwargs.get("layout", torch.strided) is not torch.strided):
                return original(*args, **kwargs)
            kw = dict(kwargs, device="meta")
            kw.pop("pin_memory", None)
            requires_grad = kw.pop("requires_grad", False)
            t = self._carve(original(*args, **kw))
            if name in ("zeros", "zeros_like", "new_zeros"):
                t.zero_()
            elif name in ("ones", "new_ones"):
                t.fill_(1)
            elif name in ("full", "new_full"):
                value = kwargs["fill_value"] if "fill_value" in kwargs else args[2 if name == "new_full" else 1]
                t.fill_(value)
            return t.requires_grad_(True) if requires_grad else t
        allocate.__name__ = name
        return allocate


@contextlib.contextmanager
def redzone(device, fill):
    """Redirect torch.empty / zeros / ones / full / empty_like / zeros_like and Tensor.new_empty / new_zeros / new_full / new_ones on ``device`` to
    carved allocations for the duration of the block; requests on another device, pinned requests and ``out=`` go to the original untouched.  The
    originals are put back on exit, also on an exception."""
    originals = {n: getattr(torch, n) for n in _FACTORIES}
    inherited = {n: getattr(torch.Tensor, n) for n in _METHODS}
    own = {n: torch.Tensor.__dict__.get(n, _MISSING) for n in _METHODS}
    rz = Redzone(device, fill, originals)
    try:
        for n in _FACTORIES:
            setattr(torch, n, rz._redirect(n, originals[n], like=n in _LIKE))
        for n in _METHODS:
            setattr(torch.Tensor, n, rz._redirect(n, inherited[n], like=True))
        yield rz
    finally:
        for n in _FACTORIES:
            setattr(torch, n, originals[n])
        for n in _METHODS:
            if own[n] is _MISSING:
                delattr(torch.Tensor, n)
            else:
                setattr(torch.Tensor, n, own[n])


def same_bits(a, b):
    """torch.equal on the bytes: NaN compares by its bits, -0.0 differs from 0.0."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(_bytes(a), _bytes(b))


def _bytes(t):
    """The elements of ``t`` in logical order as a fresh 1-D uint8 tensor (a one-element tensor keeps any stride through .contiguous())."""
    return torch.empty(t.numel(), dtype=t.dtype, device=t.device).copy_(t.detach().reshape(-1)).view(torch.uint8)


def both_fills(device, body, written=(), results_on_host=False):
    """The pattern of every row.  ``body(rz)`` places its inputs with ``rz.place``, builds its packs, calls the entry point and returns a dict of the
    documented results (tensors; a don't-care region is sliced off by the row, with the line that declares it).  Run under 0x00 and then under 0xFF:
    ``check()`` must be empty both times (no guard byte and no input changed, other than the inputs named in ``written``) and the results of the two
    runs must be equal bit for bit.  Returns the results of the 0x00 run, on the CPU."""
    runs, original = [], torch.empty
    for fill in FILLS:
        with redzone(device, fill) as rz:
            assert torch.empty is not original
            results = body(rz)
            bad = rz.check(written=written)
            assert not bad, f"fill {fill:#04x}: " + "; ".join(map(str, bad))
            if results_on_host:          # an entry point that copies its defined part to the host itself: its device buffers must still be carved
                assert any(b.clone is None for b in rz.blocks), "nothing but the inputs was allocated inside the harness: the row checks nothing"
            else:
                assert any(rz.owns(v) for v in results.values()), "no result was allocated inside the harness: the row checks nothing"
            runs.append({k: v.detach().cpu().clone() for k, v in results.items()})
        assert torch.empty is original, "harness off: allocation is what it was"
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if not same_bits(a, b):
            diff = (_bytes(a) != _bytes(b)).nonzero().flatten()
            nan_only_ff = bool(b.is_floating_point() and torch.isnan(b).any() and not torch.isnan(a).any())
            raise AssertionError(f"result {k!r} {tuple(a.shape)} {a.dtype} differs between fill 0x00 and 0xFF: {diff.numel()} byte(s), the first at "
                                 f"byte {int(diff[0])} (element {int(diff[0]) // a.element_size()})"
                                 + ("; NaN under 0xFF only" if nan_only_ff else ""))
    return runs[0]
