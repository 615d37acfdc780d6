"""tests/redzone.py proven on device="cpu" with ordinary torch code: what it carves (dtype, shape, strides, initial value, the guards flush on both
sides), what it leaves to the original functions, that it puts the originals back, and that check() sees one changed byte just past the end, just
before the start and at the far end of a guard, a changed placed input, and nothing after a clean run."""
import pytest
import torch

from redzone import FILLS, GUARD, both_fills, redzone, same_bits

CPU = torch.device("cpu")
PATCHED = [(torch, n) for n in ("empty", "zeros", "ones", "full", "empty_like", "zeros_like")] + \
          [(torch.Tensor, n) for n in ("new_empty", "new_zeros", "new_full", "new_ones")]


def _block_of(rz, t):
    (b,) = [b for b in rz.blocks if b.tensor is t]
    return b


def _is_carved(rz, t, fill):
    """``t`` is the last allocation of ``rz``: its bytes start GUARD into a uint8 block and end GUARD before the block's end, guards full of ``fill``."""
    b = rz.blocks[-1]
    assert b.tensor is t and b.base.dtype == torch.uint8 and b.base.numel() == 2 * GUARD + b.nbytes
    assert t.untyped_storage().data_ptr() == b.base.untyped_storage().data_ptr()
    assert t.storage_offset() * t.element_size() == GUARD
    extent = 0 if t.numel() == 0 else (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
    assert extent == b.nbytes                                            # the interior ends on the request's exact last byte
    assert t.data_ptr() % 64 == b.base.data_ptr() % 64                   # the interior keeps the block's alignment
    assert bool((b.base[:GUARD] == fill).all()) and bool((b.base[GUARD + b.nbytes:] == fill).all())
    return b


@pytest.mark.parametrize("fill", FILLS)
def test_shapes_as_varargs_and_tuples_and_initial_values(fill):
    with redzone(CPU, fill) as rz:
        a = torch.empty(3, 5)
        b = _is_carved(rz, a, fill)
        assert a.shape == (3, 5) and a.dtype == torch.float32 and a.is_contiguous()
        assert bool((b.base[GUARD:GUARD + b.nbytes] == fill).all()), "empty leaves the fill"
        if fill == 0xFF:
            assert torch.isnan(a).all()
        a = torch.empty((3, 5), dtype=torch.float64, device="cpu")
        _is_carved(rz, a, fill)
        assert a.shape == (3, 5) and a.dtype == torch.float64
        z = torch.zeros(7, dtype=torch.int32)
        _is_carved(rz, z, fill)
        assert z.tolist() == [0] * 7
        z = torch.zeros((2, 3), device=CPU)
        _is_carved(rz, z, fill)
        assert torch.equal(z, z * 0) and z.shape == (2, 3)
        o = torch.ones(2, 3, dtype=torch.float16)
        _is_carved(rz, o, fill)
        assert o.dtype == torch.float16 and bool((o == 1).all())
        f = torch.full((4,), 2.5)
        _is_carved(rz, f, fill)
        assert f.dtype == torch.float32 and f.tolist() == [2.5] * 4
        f = torch.full((4,), 7)
        _is_carved(rz, f, fill)
        assert f.dtype == torch.int64 and f.tolist() == [7] * 4
        f = torch.full(size=(2, 2), fill_value=-3, dtype=torch.int16)
        _is_carved(rz, f, fill)
        assert f.dtype == torch.int16 and f.flatten().tolist() == [-3] * 4
        g = torch.empty(3, requires_grad=True)
        _is_carved(rz, g, fill)
        assert g.requires_grad
        assert len(rz.blocks) == 9 and [b.ordinal for b in rz.blocks] == list(range(9))
        assert rz.check() == []


@pytest.mark.parametrize("fill", FILLS)
def test_new_methods(fill):
    src = torch.arange(6, dtype=torch.int16).view(2, 3)
    with redzone(CPU, fill) as rz:
        a = src.new_empty((4, 2))
        _is_carved(rz, a, fill)
        assert a.dtype == torch.int16 and a.shape == (4, 2)
        if fill == 0xFF:
            assert bool((a == -1).all())
        a = src.new_empty(5, dtype=torch.float32)
        _is_carved(rz, a, fill)
        assert a.dtype == torch.float32 and a.shape == (5,)
        a = src.new_zeros(2, 2)
        _is_carved(rz, a, fill)
        assert a.dtype == torch.int16 and a.flatten().tolist() == [0] * 4
        a = src.new_ones((3,))
        _is_carved(rz, a, fill)
        assert a.tolist() == [1, 1, 1]
        a = src.new_full((3,), 9)
        _is_carved(rz, a, fill)
        assert a.dtype == torch.int16 and a.tolist() == [9, 9, 9]
        assert rz.check() == []


@pytest.mark.parametrize("fill", FILLS)
def test_memory_formats_and_like_strides(fill):
    with redzone(CPU, fill) as rz:
        a = torch.empty(2, 5, 3, 4, memory_format=torch.channels_last)
        _is_carved(rz, a, fill)
        assert a.stride() == torch.empty(2, 5, 3, 4, device="meta", memory_format=torch.channels_last).stride() == (60, 1, 20, 5)
        a = torch.empty((2, 5, 3, 4, 2), memory_format=torch.channels_last_3d, dtype=torch.bfloat16)
        _is_carved(rz, a, fill)
        assert a.is_contiguous(memory_format=torch.channels_last_3d) and a.dtype == torch.bfloat16
    strided = torch.randn(4, 6, 5).permute(2, 0, 1)                       # dense, not contiguous
    assert not strided.is_contiguous()
    with redzone(CPU, fill) as rz:
        for fn in (torch.empty_like, torch.zeros_like):
            a = fn(strided)
            _is_carved(rz, a, fill)
            assert a.shape == strided.shape and a.stride() == strided.stride()
        assert bool((a == 0).all())
        a = torch.empty_like(strided, memory_format=torch.contiguous_format, dtype=torch.float16)
        _is_carved(rz, a, fill)
        assert a.is_contiguous() and a.dtype == torch.float16
        a = torch.zeros_like(torch.randn(8, 8)[:, ::2])                    # not dense: the same strides the original call gives
        _is_carved(rz, a, fill)
        assert a.shape == (8, 4) and a.is_contiguous()
        assert rz.check() == []


@pytest.mark.parametrize("fill", FILLS)
def test_zero_element_requests(fill):
    with redzone(CPU, fill) as rz:
        for make in (lambda: torch.empty(0), lambda: torch.zeros(3, 0, 4), lambda: torch.empty((0, 7), dtype=torch.int64),
                     lambda: torch.randn(0, 2).new_empty(0), lambda: torch.empty_like(torch.randn(0, 5))):
            a = make()
            b = _is_carved(rz, a, fill)
            assert a.numel() == 0 and b.nbytes == 0
        assert torch.zeros(3, 0, 4).shape == (3, 0, 4)
        assert rz.check() == []


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.bool])
def test_integer_and_half_dtypes(dtype):
    with redzone(CPU, 0xFF) as rz:
        a = torch.empty(5, 3, dtype=dtype)                                # an odd element count: the block is not a multiple of anything
        b = _is_carved(rz, a, 0xFF)
        assert a.dtype == dtype and b.nbytes == 15 * a.element_size()
        if dtype.is_floating_point:
            assert torch.isnan(a).all()
        elif dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
            assert bool((a == -1).all())
        a.zero_()
        assert rz.check() == [], "writing the whole interior touches no guard"


def test_other_device_pinned_and_out_pass_through():
    with redzone(CPU, 0xFF) as rz:
        m = torch.empty(3, device="meta")
        assert m.device.type == "meta"
        assert torch.zeros_like(m).device.type == "meta" and m.new_empty(2).device.type == "meta"
        assert torch.empty_like(torch.randn(2), device="meta").device.type == "meta"
        out = torch.arange(4.0)
        got = torch.zeros(4, out=out)
        assert got is out and out.tolist() == [0.0] * 4
        assert rz.blocks == [], "nothing above is an allocation on the guarded device"
        if torch.cuda.is_available():
            p = torch.empty(4, pin_memory=True)
            assert p.is_pinned() and rz.blocks == []
            c = torch.empty(4, device="cuda")
            assert c.is_cuda and rz.blocks == []
        on_cpu = torch.empty_like(m, device="cpu")                        # the device named in the call decides, not the source's
        assert on_cpu.device.type == "cpu" and len(rz.blocks) == 1


def test_originals_are_restored_also_after_an_exception():
    before = [getattr(o, n) for o, n in PATCHED]
    own_before = [n in o.__dict__ for o, n in PATCHED]
    with redzone(CPU, 0x00):
        assert all(getattr(o, n) is not f for (o, n), f in zip(PATCHED, before))
    assert all(getattr(o, n) is f for (o, n), f in zip(PATCHED, before)), "harness off: torch.empty is the original object"
    with pytest.raises(RuntimeError, match="inside"):
        with redzone(CPU, 0xFF):
            raise RuntimeError("inside")
    assert all(getattr(o, n) is f for (o, n), f in zip(PATCHED, before))
    assert [n in o.__dict__ for o, n in PATCHED] == own_before
    a = torch.empty(4)                                                    # and allocation is what it was: a storage of its own
    assert a.storage_offset() == 0 and a.untyped_storage().nbytes() == 16


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("where,side,offset", [("past", "guard past the end", 0), ("before", "guard before the start", GUARD - 1),
                                               ("far_end", "guard past the end", GUARD - 1), ("far_start", "guard before the start", 0)])
def test_check_reports_one_changed_guard_byte(fill, where, side, offset):
    with redzone(CPU, fill) as rz:
        torch.zeros(3)
        t = torch.empty(5, 3, dtype=torch.float16)
        torch.ones(2)
        b = _block_of(rz, t)
        at = {"past": GUARD + b.nbytes, "before": GUARD - 1, "far_end": 2 * GUARD + b.nbytes - 1, "far_start": 0}[where]
        b.base[at] = 0x5A                                                 # a stray store, through the base block
        (v,) = rz.check()
        assert (v.kind, v.ordinal, v.shape, v.dtype, v.side, v.offset, v.count) == ("guard byte changed", 1, (5, 3), torch.float16, side, offset, 1)
        assert "allocation #1" in str(v) and side in str(v)


def test_check_counts_a_vector_store_past_a_ragged_tail():
    with redzone(CPU, 0x00) as rz:
        t = torch.empty(25)
        b = _block_of(rz, t)
        b.base[GUARD:].view(torch.float32)[24:28] = 1.0                   # a float4 at element 24 of 25
        (v,) = rz.check()
        assert (v.side, v.offset, v.count) == ("guard past the end", 2, 6)      # 1.0f = 00 00 80 3f: two of four bytes differ from 0x00
        assert t[24] == 1.0


@pytest.mark.parametrize("fill", FILLS)
def test_check_reports_a_changed_placed_input(fill):
    src = torch.randn(3, 4, 5).permute(2, 0, 1)
    with redzone(CPU, fill) as rz:
        x = rz.place(src, name="x")
        w = rz.place(torch.arange(7, dtype=torch.int32))
        b = _is_carved(rz, w, fill)
        assert b.clone is not None and torch.equal(x, src) and x.stride() == src.stride() and x.data_ptr() != src.data_ptr()
        ragged = rz.place(torch.randn(8, 8)[:, ::2])                      # not dense: placed in its contiguous form
        assert ragged.is_contiguous() and ragged.shape == (8, 4)
        assert rz.check() == []
        x[1, 2, 3] += 1.0
        (v,) = rz.check()
        assert (v.kind, v.ordinal, v.name, v.side) == ("input changed", 0, "x", "interior") and 1 <= v.count <= 4
        assert rz.check(written=("x",)) == [] and rz.check(written=(x,)) == [], "an input the op documents as written in place"
        w[6] = -1
        assert [v.ordinal for v in rz.check(written=("x",))] == [1]
        assert x[1, 2, 3] == src[1, 2, 3] + 1.0, "place copies: the caller's tensor is not the placed one"


def test_same_bits_compares_nan_by_bits():
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32)) and not same_bits(torch.zeros(2), torch.zeros(3))
    assert same_bits(torch.empty(0), torch.empty(0))
    odd = torch.arange(18.0).view(2, 9)[:1, 7]                             # one element, stride 9: .contiguous() leaves it as it is
    assert odd.stride() == (9,) and same_bits(odd, torch.tensor([7.0])) and not same_bits(odd, torch.tensor([8.0]))


def test_both_fills_on_plain_torch_code():
    """The row pattern on ordinary CPU code: a clean op passes; an op that leaves an output element unset, one that reads past its input, and one that
    stores past its output each fail in the way the GPU rows are meant to catch."""
    src = torch.randn(6, 5)

    def clean(rz):
        x = rz.place(src)
        y = torch.empty(6, 5)
        torch.mul(x, 2.0, out=y)
        return {"y": y}
    got = both_fills(CPU, clean)
    assert torch.equal(got["y"], src * 2.0)

    def unset_tail(rz):
        x = rz.place(src)
        y = torch.empty(6, 5)
        y.view(-1)[:29] = x.view(-1)[:29]
        return {"y": y}
    with pytest.raises(AssertionError, match="differs between fill 0x00 and 0xFF.*element 29.*NaN under 0xFF only"):
        both_fills(CPU, unset_tail)

    def reads_slack(rz):
        x = rz.place(src)
        beyond = rz.blocks[-1].base[GUARD:].view(torch.float32)[:32]      # a K-tail read two elements past the 30 of x
        y = torch.empty(1)
        y[0] = (beyond * torch.tensor([1.0] * 30 + [0.0] * 2)).sum()
        return {"y": y}
    with pytest.raises(AssertionError, match="NaN under 0xFF only"):
        both_fills(CPU, reads_slack)

    def stray_store(rz):
        y = torch.zeros(30)
        rz.blocks[-1].base[GUARD:].view(torch.float32)[28:32] = 0.0      # a float4 at the ragged tail: invisible over 0x00 slack
        return {"y": y}
    with pytest.raises(AssertionError, match="fill 0xff: guard byte changed.*past the end.*8 byte"):
        both_fills(CPU, stray_store)

    def scribbles(rz):
        x = rz.place(src, name="x")
        x.mul_(2.0)
        return {"y": x}
    with pytest.raises(AssertionError, match="input changed"):
        both_fills(CPU, scribbles)
    assert torch.equal(both_fills(CPU, scribbles, written=("x",))["y"], src * 2.0)

    with pytest.raises(AssertionError, match="no result was allocated inside the harness"):
        both_fills(CPU, lambda rz: {"y": src + 1.0})
    with redzone(CPU, 0x00) as rz:
        assert rz.owns(torch.empty(3)[1:]) and rz.owns(rz.place(src)) and not rz.owns(src)
