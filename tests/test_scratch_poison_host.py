"""tests/scratch_poison.py on CPU tensors (device="cpu"): the fills' bytes, the guards, "keep", and that the three replaced names come
back.  The GPU contract test (tests/test_gpu_scratch_contract.py) relies on every one of these.

"keep" reads whether a buffer is still held from torch._C._storage_Use_Count, a private torch API: test_keep_pins_the_storage_use_count
pins the behaviour the helper needs of it, and that the helper refuses to run when it is gone."""
import pytest
import torch

from diffab_pytorch import _hip
from scratch_poison import FILL_BYTE, GUARD, GUARD_BYTE, GuardDamaged, poisoned, raw_bytes

DTYPES = [torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool]


def _names():
    return _hip.workspace, torch.empty, torch.empty_like


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("fill", ["zero", "ff"])
def test_constant_fills(fill, dtype):
    with poisoned(fill, device="cpu") as p:
        a = torch.empty(5, 7, dtype=dtype)
        b = torch.empty_like(torch.ones(3, 4, dtype=dtype).t())  # (a non-contiguous pattern: empty_like keeps its strides)
        ws = _hip.workspace(1000)
        for t in (a, b):
            raw = raw_bytes(t)
            assert raw.numel() == t.numel() * t.element_size()
            assert bool((raw == FILL_BYTE[fill]).all()), (fill, dtype)
        assert bool((ws == FILL_BYTE[fill]).all())
        assert a.shape == (5, 7) and a.dtype == dtype and b.shape == (4, 3) and ws.shape == (1000,) and ws.dtype == torch.uint8
        if fill == "ff":
            if dtype == torch.float32:
                assert bool(a.isnan().all())
            elif dtype in (torch.int64, torch.int32):
                assert bool((a == -1).all())
            elif dtype == torch.bool:
                assert bool(a.all())
        else:
            assert not bool(a.any())
        p.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_random_fill_is_seeded_bytes(dtype):
    def draw(seed):
        with poisoned("random", seed=seed, device="cpu"):
            return raw_bytes(torch.empty(64, 33, dtype=dtype)).clone(), _hip.workspace(5000).clone()

    a, wa = draw(3)
    b, wb = draw(3)
    c, _ = draw(4)
    assert torch.equal(a, b) and torch.equal(wa, wb) and not torch.equal(a, c)
    for raw in (a, wa):  # bytes, not values of the dtype: every byte value occurs (2112+ draws of 256 values)
        assert raw.unique().numel() > 200
    if dtype == torch.float32:
        v = a.view(torch.float32)
        assert bool((v.abs() > 1e30).any()) and bool(((v.abs() < 1e-30) & (v != 0)).any())  # huge and tiny floats


def test_workspace_is_aligned_and_at_least_256_bytes():
    with poisoned("zero", device="cpu") as p:
        ws = _hip.workspace(10)
        assert ws.numel() == 256
        base = p.bases[0][0]
        assert base.numel() == 256 + 2 * GUARD
        assert ws.data_ptr() - base.data_ptr() == GUARD and GUARD % 256 == 0
        assert bool((base[:GUARD] == GUARD_BYTE).all()) and bool((base[GUARD + 256:] == GUARD_BYTE).all())


@pytest.mark.parametrize("where, offset", [("before", -1), ("after", 3000), ("far_before", -GUARD), ("far_after", 3000 + GUARD - 1)])
def test_a_write_outside_the_interior_is_caught_with_its_offset(where, offset):
    with pytest.raises(GuardDamaged) as err:
        with poisoned("ff", device="cpu") as p:
            _hip.workspace(512)
            _hip.workspace(3000)
            _hip.workspace(512)
            p.bases[1][0][GUARD + offset] = 0  # through the base buffer: the byte at `offset` from the second interior's start
    assert "3000 bytes" in str(err.value) and f"offset {offset} " in str(err.value), str(err.value)


def test_check_can_be_called_inside_and_a_clean_run_passes():
    with poisoned("random", device="cpu") as p:
        ws = _hip.workspace(777)
        ws[:] = 1  # the whole interior, first and last byte included
        p.check()
        p.bases[0][0][GUARD - 1] = 7
        with pytest.raises(GuardDamaged, match="offset -1 "):
            p.check()
        p.bases[0][0][GUARD - 1] = GUARD_BYTE


def test_names_are_restored_after_a_normal_exit_and_after_an_exception():
    before = _names()
    with poisoned("zero", device="cpu"):
        assert all(a is not b for a, b in zip(_names(), before))
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(KeyError):
        with poisoned("ff", device="cpu"):
            raise KeyError("from the body")
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(GuardDamaged):  # the exit's own failure restores them too
        with poisoned("ff", device="cpu") as p:
            _hip.workspace(300)
            p.bases[0][0][0] = 0
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(ValueError):
        poisoned("nan")


def test_keep_hands_the_leftover_to_the_next_request():
    with poisoned("keep", device="cpu") as p:
        a = _hip.workspace(2048)
        assert not bool(a.any())  # a new buffer starts as zeros
        a[:] = torch.arange(2048) % 251
        where = a.data_ptr()
        held = _hip.workspace(2048)  # `a` is still held: never the same memory twice at once
        assert held.data_ptr() != where
        held[:] = 9
        del a
        b = _hip.workspace(2048)  # the same size again, nobody holds the first: the same storage with its contents
        assert b.data_ptr() == where and torch.equal(b, (torch.arange(2048) % 251).to(torch.uint8))
        del b
        c = _hip.workspace(1000)  # a smaller request: the front of a kept buffer
        assert c.data_ptr() == where and torch.equal(c, (torch.arange(1000) % 251).to(torch.uint8))
        big = _hip.workspace(4096)  # nothing kept is large enough
        assert not bool(big.any()) and len(p.bases) == 3
        e = torch.empty(16)  # torch.empty is left alone under "keep"
        assert e.shape == (16,)


def test_keep_pins_the_storage_use_count(monkeypatch):
    """One holder per view, also for a view that only an autograd node holds; and "keep" raises, not reallocates, when the count stops
    moving."""
    import scratch_poison

    base = torch.zeros(64, dtype=torch.uint8)
    idle = scratch_poison._holders(base)
    view = base[8:16]
    assert scratch_poison._holders(base) == idle + 1
    other = view.view(torch.int32)
    assert scratch_poison._holders(base) == idle + 2
    del view, other
    assert scratch_poison._holders(base) == idle
    monkeypatch.setattr(scratch_poison, "_holders", lambda base: 2)
    with pytest.raises(RuntimeError, match="_storage_Use_Count"):
        with poisoned("keep", device="cpu"):
            _hip.workspace(512)
    with poisoned("zero", device="cpu"):  # the other fills never ask
        _hip.workspace(512)


def test_keep_sees_a_tensor_saved_for_backward_as_held():
    class Taped(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            tape = _hip.workspace(512)
            tape[:] = 5
            ctx.save_for_backward(tape)
            return x * 2

        @staticmethod
        def backward(ctx, g):
            (tape,) = ctx.saved_tensors
            assert bool((tape == 5).all())
            return g * 2

    with poisoned("keep", device="cpu") as p:
        x = torch.ones(3, requires_grad=True)
        y1 = Taped.apply(x)
        y2 = Taped.apply(x)  # two tapes of one size alive at once
        assert len(p.bases) == 2
        _hip.workspace(512)[:] = 1  # a third request while both are held
        (y1.sum() + y2.sum()).backward()
        assert len(p.bases) == 3 and torch.equal(x.grad, torch.full((3,), 4.0))


def test_other_devices_out_forms_and_meta_pass_untouched():
    class ElsewherePoisoned(poisoned):  # the target is a GPU this machine need not have: nothing here may touch it
        device = torch.device("cuda", 0)

        def _fill_bytes(self, u8, fill):
            raise AssertionError("a tensor off the target device was filled")

    with ElsewherePoisoned("ff"):
        a = torch.empty(4, 4)
        a.fill_(2.0)
        b = torch.empty_like(a)
        assert a.device.type == "cpu" and b.shape == (4, 4)
        m = torch.empty(8, device="meta")
        assert m.device.type == "meta"
    with poisoned("ff", device="cpu"):
        out = torch.full((6,), 3.0)
        got = torch.empty(6, out=out)
        assert got is out and bool((out == 3.0).all())  # an out= form keeps what the caller's tensor held
        fresh = torch.empty(6)
        assert bool(fresh.isnan().all())
        m = torch.empty(8, device="meta")
        assert m.device.type == "meta"
